// Surrogate inference of MFM_missing (include/mfm_hip.h, mfm_impute_missing): a missing modality m and the label from the other
// two modalities -- decoded_no<m>[index of m] and decoded_no<m>[3] of the class's forward (mfm_model.py:766-885) in eval mode --
// on what they depend on alone: the two surrogate encoders that read the observed pair (-> z_m', -> zy'), zy_to_fy, z{m}_to_f{m},
// decoder_m and fy_to_y.  No MFN, no own-modality encoder, no other decoder.  The pattern of the inference launches
// (infer_dev.h): the recurrence with small_fwd_body<.., REC = false>, h / c on chip, the row-wise layers (dense_rows_dev.h) in the
// workgroup that holds the rows.
//
// Per row chunk and for the cases asked for (one of l / a / v, or all three):
//   0. impute_gather_kernel copies the observed pair of every case -- (a, v), (l, v), (l, a): the columns of x without those of
//      m -- into the workspace as a matrix of its own, rows padded with zeros.  The GEMM fetches 16 bytes at a time and masks
//      what lies beyond a row's K range by MULTIPLYING with zero (gemm.hip): on a column range of x that fetch would meet the
//      neighbouring columns, which are those of the missing modality (la: v behind it; av: l of the next row), and a NaN there
//      would survive the mask.  On the gathered copy it meets the padding;
//   1. the input projections of the 2 (6) surrogate encoders as ONE grouped fp32 GEMM on the gathered pairs (the two encoders
//      of a case share theirs);
//   2. impute_encode_kernel: workgroup (encoder e, row tile) runs e's T-step recurrence and then e's fc1 on the tile's last hidden
//      states still in LDS; it writes its rows of z (plain encoderLSTMs: no mean / logvar heads);
//   3. decode_factors_kernel (generate.hip): workgroup (case m, row tile) computes fy = relu(zy_to_fy_fc2(relu(zy_to_fy_fc1(zy'_m))))
//      and f_m likewise from z_m' into LDS, the classifier on fy -> y_hat_m, and runs the decoder form of the recurrence on
//      [fy | f_m] storing h_t alone.  Every case has its OWN zy' and its own y_hat;
//   4. the decoders' fc1 over the stored h as one grouped fp32 GEMM straight into x_hat_m.
// The z rows travel through HBM between launches 2 and 3 (stream order: no flag, no workgroup waits for another).  Launches 2
// and 3 follow the launch rules of infer_dev.h: the per-block switch is instantiated for the canonical size tuples only (the
// encoders: one per case, one for all three cases), any other combination takes one launch per LSTM of the same kernel.
#include "infer_dev.h"

namespace mfm {

__global__ __launch_bounds__(256) void impute_gather_kernel(const ImpGather G) {
  const int c = blockIdx.y;
  const int ld = G.ld[c], k = G.k[c], s0 = G.s0[c], len0 = G.len0[c], s1 = G.s1[c];
  float* __restrict__ out = G.out[c];
  const int64_t total = (int64_t)G.T * G.n * ld;      // (< 2^31: checked by the host; 64 bits: the last stride may pass that)
  for (int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i64 < total; i64 += (int64_t)gridDim.x * blockDim.x) {
    const int idx = (int)i64, row = idx / ld, j = idx - row * ld;
    const int t = row / G.n, i = row - t * G.n;
    out[idx] = (j < k) ? G.x[((int64_t)t * G.N + G.n0 + i) * G.D + (j < len0 ? s0 + j : s1 + j - len0)] : 0.0f;
  }
}

template <int R, int K0, int K1, int K2, int K3, int K4, int K5>
__global__ __launch_bounds__(1024) void impute_encode_kernel(const ImpEncodeDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, bid = blockIdx.x;
  MFM_SEQ_BLOCK_LSTM(P, bid, di)
  const ImpEnc& E = P.d[di];
  const int tile = bid - E.block_begin, b0 = tile * R;
  const float* hT = nullptr;
  MFM_TUPLE6(hT = small_fwd_body<KQ, R, false, false, false>(E.seq, P.T, P.n, tile, lds))
  // the two h buffers stay where they are; fc1's output behind them ([maxw][R])
  float* act0 = lds + 2 * E.seq.Hp * R;
  const int h = E.seq.h;
  dense_rows<R>(E.w, E.b, h, h, hT, act0, false);
  store_rows<R>(act0, E.z, h, b0, P.n, tid);
}

// ---------------------------------------------------------------- host
bool imp_sizes(const int32_t* sz, int cases, ImpSizes& S) {
  for (int i = 0; i < 12; ++i)
    if (sz[i] < 1) return false;
  if (cases != 1 && cases != 2 && cases != 4 && cases != 7) return false;
  for (int m = 0; m < IMP_CASES; ++m) { S.z[m] = sz[m]; S.fm[m] = sz[4 + m]; S.dm[m] = sz[8 + m]; }
  S.zy = sz[3]; S.fy = sz[7]; S.od = sz[11];
  S.D = S.dm[0] + S.dm[1] + S.dm[2];
  S.din[0] = S.dm[1] + S.dm[2]; S.din[1] = S.dm[0] + S.dm[2]; S.din[2] = S.dm[0] + S.dm[1];
  // a 16-byte fetch clamped to the last column reaches 3 floats past it: they must be the row's own padding
  for (int m = 0; m < IMP_CASES; ++m) S.ld[m] = (S.din[m] + 3) / 4 * 4 + 4;
  S.nc = 0;
  for (int m = 0; m < IMP_CASES; ++m)
    if (cases >> m & 1) S.cs[S.nc++] = m;
  return true;
}


// workspace of one chunk, in floats, every part a multiple of 4: per case the two encoders' x-projections, the two z rows, the
// decoder's stored h and the gathered pair
static int64_t imp_ws_floats(int64_t T, int64_t N, const ImpSizes& S, int64_t max_rows) {
  const int64_t rows = gen_rows(N, max_rows);
  int64_t f = 0;
  for (int c = 0; c < S.nc; ++c) {
    const int m = S.cs[c];
    f += rows * T * 4 * (hp_of(S.z[m]) + hp_of(S.zy)) + up4(rows * S.z[m]) + up4(rows * S.zy) + rows * T * hp_of(S.fy + S.fm[m])
         + rows * T * S.ld[m];
  }
  return f;
}

static const int kImpEnc[IMP_ENC] = {8, 8, 2, 8, 20, 8};     // the canonical sizes: encoders -> z_m h = 32 / 8 / 80, -> zy h = 32

// the launch(es) of one chunk of n rows (infer_launch_tuple_or_each); P.d holds the encoders of the cases asked for, two per
// case; m0: the case when it is one
template <int R>
static int imp_encode_launch(const char* who, ImpEncodeDev& P, int m0, int threads, size_t lds_bytes, hipStream_t stream) {
  const int ne = P.count;
  bool canon = true;
  for (int i = 0; i < ne; ++i) canon = canon && P.d[i].seq.hk4 == kImpEnc[ne == IMP_ENC ? i : 2 * m0 + i];
  void (*kernel)(const ImpEncodeDev) = nullptr;
  if (canon && ne == IMP_ENC) kernel = impute_encode_kernel<R, 8, 8, 2, 8, 20, 8>;
  else if (canon && m0 == 0) kernel = impute_encode_kernel<R, 8, 8, 0, 0, 0, 0>;
  else if (canon && m0 == 1) kernel = impute_encode_kernel<R, 2, 8, 0, 0, 0, 0>;
  else if (canon) kernel = impute_encode_kernel<R, 20, 8, 0, 0, 0, 0>;
  return infer_launch_tuple_or_each<R>(who, "impute_encode_kernel", P, kernel,
                                       [](auto kk) { return impute_encode_kernel<R, decltype(kk)::value, 0, 0, 0, 0, 0>; }, threads, lds_bytes, stream);
}

// the same with the encoders -> z_m alone, one per case: the three of the canonical sizes in one launch, anything else (one case
// among them) one launch per LSTM of the per-size instantiation
template <int R>
static int imp_encode_launch_z(const char* who, ImpEncodeDev& P, int threads, size_t lds_bytes, hipStream_t stream) {
  bool canon = P.count == IMP_CASES;
  for (int i = 0; canon && i < IMP_CASES; ++i) canon = P.d[i].seq.hk4 == kImpEnc[2 * i];
  return infer_launch_tuple_or_each<R>(who, "impute_encode_kernel", P, canon ? impute_encode_kernel<R, 8, 2, 20, 0, 0, 0> : nullptr,
                                       [](auto kk) { return impute_encode_kernel<R, decltype(kk)::value, 0, 0, 0, 0, 0>; }, threads, lds_bytes, stream);
}

int impute_encode_launch(const char* who, ImpEncodeDev& P, bool pairs, int m0, int R, int threads, size_t lds_bytes, hipStream_t stream) {
  if (pairs) return (R == 1) ? imp_encode_launch<1>(who, P, m0, threads, lds_bytes, stream) : imp_encode_launch<4>(who, P, m0, threads, lds_bytes, stream);
  return (R == 1) ? imp_encode_launch_z<1>(who, P, threads, lds_bytes, stream) : imp_encode_launch_z<4>(who, P, threads, lds_bytes, stream);
}

void imp_gather_case(ImpGather& G, int c, int m, const ImpSizes& S, float* out) {
  G.out[c] = out;
  G.k[c] = S.din[m]; G.ld[c] = S.ld[m];
  G.s0[c] = m == 0 ? S.dm[0] : 0; G.len0[c] = m == 1 ? S.dm[0] : S.din[m]; G.s1[c] = S.dm[0] + S.dm[1];
}

int impute_gather_launch(const ImpGather& G, int nc, hipStream_t stream) {
  const int gblocks = (int)std::min<int64_t>(((int64_t)G.T * G.n * (G.D + 4) + 255) / 256, 4 * device_cus());
  impute_gather_kernel<<<dim3(gblocks, nc), dim3(256), 0, stream>>>(G);
  MFM_LAUNCH_CHECK("impute_gather_kernel");
  return MFM_OK;
}

static int impute_missing(int T, int64_t N, const int32_t* sz, int cases, const float* const* prm, const float* x, float* ws,
                          float* const* out, int64_t max_rows, hipStream_t stream) {
  static const char* who = "impute missing";
  MFM_REQUIRE(sz && prm && x && ws && out, "%s: bad arguments (sizes, parameter table, x, workspace and outputs must not be null)", who);
  int rc = infer_check_sizes(who, T, N, sz);
  if (rc != MFM_OK) return rc;
  MFM_REQUIRE(cases == 1 || cases == 2 || cases == 4 || cases == 7, "%s: cases = %d (bit 0 l, bit 1 a, bit 2 v: one of them, or all three)", who, cases);
  if ((rc = infer_check_rows(who, N, max_rows)) != MFM_OK) return rc;
  // (x is read by the gather alone, element by element; the GEMMs and the recurrences read the workspace 16 bytes at a time)
  MFM_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)ws & 15) == 0, "%s: x must be 4-byte aligned, the workspace 16-byte aligned", who);
  ImpSizes S;
  imp_sizes(sz, cases, S);
  for (int c = 0; c < S.nc; ++c) {
    const int m = S.cs[c];
    for (int i = 0; i < IMP_CASE_PTRS; ++i) {
      const float* p = prm[m * IMP_CASE_PTRS + i];
      MFM_REQUIRE(p, "%s: parameter %d of case %d is null", who, i, m);
      const bool lstm_w = i == 0 || i == 1 || i == 6 || i == 7 || i == 16 || i == 17;
      MFM_REQUIRE(((uintptr_t)p & (lstm_w ? 15 : 3)) == 0, "%s: parameter %d of case %d is misaligned (LSTM weights 16 bytes, the rest 4)", who, i, m);
    }
    MFM_REQUIRE(out[2 * m] && out[2 * m + 1], "%s: an output of case %d is null", who, m);
  }
  for (int i = IMP_CASES * IMP_CASE_PTRS; i < IMP_NPARAM; ++i)
    MFM_REQUIRE(prm[i] && ((uintptr_t)prm[i] & 3) == 0, "%s: shared parameter %d is null or misaligned", who, i - IMP_CASES * IMP_CASE_PTRS);

  const int rows = (int)gen_rows(N, max_rows);
  const int Re = gen_tile_rows(2 * S.nc, rows), Rd = gen_tile_rows(S.nc, rows);
  int enc_maxw = 1, enc_threads = 64, dec_maxw = std::max(std::max(S.zy, S.fy), S.od), dec_threads = 64, maxd = 1, maxhp = 16;
  size_t enc_floats = 0, dec_seq = 0;
  for (int c = 0; c < S.nc; ++c) {
    const int m = S.cs[c];
    const int hs[3] = {S.z[m], S.zy, S.fy + S.fm[m]};
    for (int i = 0; i < 3; ++i)
      if ((rc = infer_check_resident(who, hs[i])) != MFM_OK) return rc;
    enc_maxw = std::max(enc_maxw, std::max(hs[0], hs[1]));
    enc_threads = std::max(enc_threads, 8 * round_up(std::max(hs[0], hs[1]), 16));
    dec_maxw = std::max(dec_maxw, std::max(hs[2], std::max(S.z[m], S.fm[m])));
    dec_threads = std::max(dec_threads, 8 * round_up(hs[2], 16));
    dec_seq = std::max(dec_seq, seq_lds_floats(hs[2], Rd));
    maxd = std::max(maxd, std::max(S.dm[m], S.ld[m]));
    maxhp = std::max(maxhp, round_up(std::max(std::max(hs[0], hs[1]), hs[2]), 16));
  }
  for (int c = 0; c < S.nc; ++c)
    for (int i = 0; i < 2; ++i) enc_floats = std::max(enc_floats, enc_lds_floats(i ? S.zy : S.z[S.cs[c]], Re, 1, enc_maxw));
  const size_t enc_lds = lds_bytes_of(enc_floats), dec_lds = lds_bytes_of(dec_seq + (size_t)5 * dec_maxw * Rd);
  if ((rc = infer_check_lds(who, std::max(enc_lds, dec_lds), std::max(enc_maxw, dec_maxw), enc_lds > dec_lds ? Re : Rd)) != MFM_OK) return rc;
  if ((rc = infer_check_chunk(who, rows, T, std::max(std::max(S.D, maxd), 4 * maxhp), "product")) != MFM_OK) return rc;

  ImpEncodeDev PE;
  DecodeDev PD;
  memset(&PE, 0, sizeof(PE));
  memset(&PD, 0, sizeof(PD));
  const float* fcw[IMP_CASES]; const float* fcb[IMP_CASES];
  float* zbuf[IMP_CASES][2];
  ImpGather G;
  memset(&G, 0, sizeof(G));
  G.x = x; G.N = N; G.T = T; G.D = S.D;
  float* w0 = ws;
  for (int c = 0; c < S.nc; ++c) {
    const int m = S.cs[c];
    const float* const* p = prm + m * IMP_CASE_PTRS;
    for (int i = 0; i < 2; ++i) {
      ImpEnc& E = PE.d[2 * c + i];
      seq_fill(E.seq, p[6 * i], p[6 * i + 1], p[6 * i + 2], p[6 * i + 3], i ? S.zy : S.z[m], 0);
      E.seq.gates = w0; w0 += (int64_t)rows * T * 4 * E.seq.Hp;
      E.w = p[6 * i + 4]; E.b = p[6 * i + 5];
    }
    for (int i = 0; i < 2; ++i) { zbuf[c][i] = w0; w0 += up4((int64_t)rows * (i ? S.zy : S.z[m])); }
    DecOne& Dd = PD.d[c];
    seq_fill(Dd.seq, p[16], p[17], p[18], p[19], S.fy + S.fm[m], 1);
    fcw[c] = p[20]; fcb[c] = p[21];
    Dd.seq.hs = w0; w0 += (int64_t)rows * T * Dd.seq.Hp;
    for (int l = 0; l < 2; ++l) { Dd.w[l] = p[12 + 2 * l]; Dd.b[l] = p[13 + 2 * l]; }
    Dd.zs = S.z[m]; Dd.fm = S.fm[m];
    imp_gather_case(G, c, m, S, w0); w0 += (int64_t)rows * T * S.ld[m];
  }
  for (int l = 0; l < 4; ++l) { PD.wy[l] = prm[IMP_CASES * IMP_CASE_PTRS + 2 * l]; PD.by[l] = prm[IMP_CASES * IMP_CASE_PTRS + 2 * l + 1]; }
  PE.count = 2 * S.nc; PE.T = T; PE.maxw = enc_maxw;
  PD.count = S.nc; PD.T = T; PD.zys = S.zy; PD.fy = S.fy; PD.od = S.od; PD.maxw = dec_maxw; PD.seq_floats = (int)dec_seq;

  for (int64_t n0 = 0; n0 < N; n0 += rows) {
    const int n = (int)std::min<int64_t>(rows, N - n0);
    const bool whole = n == N;           // one chunk: the T * N rows of an output are one matrix
    G.n0 = n0; G.n = n;
    if ((rc = impute_gather_launch(G, S.nc, stream)) != MFM_OK) return rc;
    // gates_e[t][i][g][u] = pair_e[t][i] . W_ih[g h + u] + b_ih + b_hh; pad units u >= h exact zeros.  The gathered pair of a
    // chunk is one [T * n, ld] matrix whatever the chunk
    rc = gemm_group_each(PE.count, stream, [&](int e, MfmGemmDesc& d) {
      const int c = e / 2;
      xproj_desc(d, PE.d[e].seq, G.out[c], G.ld[c], G.k[c], T * n, PE.d[e].seq.gates);
    });
    if (rc != MFM_OK) return rc;
    PE.n = PD.n = n;
    for (int c = 0; c < S.nc; ++c) {
      const int m = S.cs[c];
      PE.d[2 * c].z = zbuf[c][0]; PE.d[2 * c + 1].z = zbuf[c][1];
      PD.d[c].zm = zbuf[c][0]; PD.d[c].zy = zbuf[c][1];
      PD.d[c].y_hat = out[2 * m + 1] + n0 * S.od;
    }
    rc = impute_encode_launch(who, PE, true, S.cs[0], Re, enc_threads, enc_lds, stream);
    if (rc != MFM_OK) return rc;
    rc = decode_factors_launch(who, PD, Rd, dec_threads, dec_lds, stream);
    if (rc != MFM_OK) return rc;
    // x_hat_m[t][n0 + i] = hs_m[t][i] . Wfc_m^T + b: one problem per case -- the whole split as one matrix, a chunk as T batched
    // products (the stored h of a chunk is [T][n, Hp], its rows of x_hat_m lie N rows apart per step)
    rc = gemm_group_each(PD.count, stream, [&](int c, MfmGemmDesc& d) {
      const int m = S.cs[c];
      const SeqDev& s = PD.d[c].seq;
      dec_fc1_desc(d, s, s.hs, fcw[c], fcb[c], out[2 * m] + n0 * S.dm[m], S.dm[m], whole ? T * n : n, whole ? 1 : T, (int64_t)n * s.Hp,
                   N * S.dm[m]);
    });
    if (rc != MFM_OK) return rc;
  }
  return MFM_OK;
}

}  // namespace mfm

extern "C" int64_t mfm_impute_missing_workspace_floats(int32_t T, int64_t N, const int32_t* sizes, int32_t cases, int64_t max_rows) {
  mfm::ImpSizes S;
  if (T < 1 || N < 1 || !sizes || max_rows < 0 || !mfm::imp_sizes(sizes, cases, S)) return 0;
  return mfm::imp_ws_floats(T, N, S, max_rows);
}

extern "C" int mfm_impute_missing_tile_rows(int64_t N, int32_t cases, int64_t max_rows, int32_t* tile_rows) {
  if (N < 1 || max_rows < 0 || !tile_rows || (cases != 1 && cases != 2 && cases != 4 && cases != 7)) {
    mfm::set_error("impute missing tile rows: bad arguments (N %lld, cases %d, row cap %lld)", (long long)N, cases, (long long)max_rows);
    return MFM_ERR_ARG;
  }
  const int nc = cases == 7 ? 3 : 1, rows = (int)std::min<int64_t>(mfm::gen_rows(N, max_rows), INT32_MAX);
  tile_rows[0] = mfm::gen_tile_rows(2 * nc, rows);
  tile_rows[1] = mfm::gen_tile_rows(nc, rows);
  return MFM_OK;
}

extern "C" int mfm_impute_missing(int32_t T, int64_t N, const int32_t* sizes, int32_t cases, const float* const* params,
                                  const float* x, float* workspace, float* const* out, int64_t max_rows, void* stream) {
  return mfm::impute_missing(T, N, sizes, cases, params, x, workspace, out, max_rows, (hipStream_t)stream);
}
