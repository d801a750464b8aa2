// The factorized latents and generation from them (include/mfm_hip.h, mfm_encode_klef / mfm_decode_factors): the two halves of
// the eval-mode forward (mfm_model.py:619-660) as calls of their own -- no plan, no training workspace, nothing a backward would
// read leaves the chip.  The pattern of the inference launches (infer_dev.h): the recurrence with small_fwd_body<.., REC = false>,
// h / c on chip, the row-wise layers (dense_rows_dev.h) in the same workgroup.
//
// mfm_encode_klef, per row chunk:
//   1. the input projections of the four encoders (l, a, v on their column ranges of x, the ef encoder on all of x) as ONE
//      grouped fp32 GEMM (one problem per encoder; a chunk that is not the whole split: one per encoder and time step);
//   2. encode_klef_kernel: workgroup (encoder e, row tile) runs e's T-step recurrence and then, on the tile's last hidden
//      states still in LDS, e's fc1, the mean head and the logvar head; it writes its rows of z_e / logvar_z_e.
// mfm_decode_factors, per row chunk:
//   1. decode_factors_kernel: workgroup (decoder m, row tile) computes fy = relu(zy_to_fy_fc2(relu(zy_to_fy_fc1(zy)))) and its
//      own f_m for its rows into LDS -- the three decoders' workgroups recompute fy on the same code path from the same inputs,
//      bit-identical -- and runs the decoder form of the recurrence on [fy | f_m] from LDS (step 0: W_ih on the embedding, then
//      W_ih + W_hh on h); h_t alone is stored (small_fwd_body's HS mode); decoder l's workgroups also run the classifier on fy
//      and write y_hat.  Every decoder carries its own zy and y_hat pointer: mfm_impute_missing (impute.hip) launches the same
//      kernel with a zy and a y_hat per case;
//   2. the three decoders' fc1 over the stored h as one grouped fp32 GEMM straight into x_hat_m.
// One launch for all encoders (decoders): the T-step chain is a latency chain and launches of one stream run one behind the
// other, so four launches would cost the sum of the four chains where one costs the longest.  The price is that every
// workgroup gets the block size and the LDS of the widest LSTM; at one-row tiles that is 11 KB and 16 waves, and two
// workgroups still fit a CU.  The per-block switch is instantiated for the canonical size tuples only; any other size
// combination takes one launch per LSTM of the same kernel (the launch rules of infer_dev.h).
#include "infer_dev.h"

namespace mfm {

#define GEN_ENC INFER_ENC
#define GEN_DEC INFER_DEC

template <int R, int K0, int K1, int K2, int K3>
__global__ __launch_bounds__(1024) void encode_klef_kernel(const EncodeDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, bid = blockIdx.x;
  MFM_SEQ_BLOCK_LSTM(P, bid, di)
  const EncOne& E = P.d[di];
  const int tile = bid - E.block_begin, b0 = tile * R;
  const float* hT = nullptr;
  MFM_TUPLE4(hT = small_fwd_body<KQ, R, false, false, false>(E.seq, P.T, P.n, tile, lds))
  // the two h buffers stay where they are; fc1's output and the two heads' behind them ([maxw][R] each)
  float* act0 = lds + 2 * E.seq.Hp * R;
  float* act1 = act0 + P.maxw * R;
  float* act2 = act1 + P.maxw * R;
  const int h = E.seq.h, zs = E.zs;
  dense_rows<R>(E.w[0], E.b[0], h, h, hT, act0, false);
  dense_rows<R>(E.w[1], E.b[1], h, zs, act0, act1, false);
  dense_rows<R>(E.w[2], E.b[2], h, zs, act0, act2, false);
  store_rows<R>(act1, E.mu, zs, b0, P.n, tid);
  store_rows<R>(act2, E.lv, zs, b0, P.n, tid);
}

template <int R, int K0, int K1, int K2>
__global__ __launch_bounds__(1024) void decode_factors_kernel(const DecodeDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, bid = blockIdx.x;
  MFM_SEQ_BLOCK_LSTM(P, bid, di)
  const DecOne& D = P.d[di];
  const int tile = bid - D.block_begin, b0 = tile * R;
  const int h = D.seq.h, fy = P.fy;
  // behind everything the recurrence uses: the embedding must survive its weight staging
  float* zin = lds + P.seq_floats;             // [maxw][R] each
  float* t0 = zin + P.maxw * R;
  float* t1 = t0 + P.maxw * R;
  float* cat = t1 + P.maxw * R;                // [fy | f_m] as [h][R]
  float* emb = cat + P.maxw * R;               // the same as [R][h]: the recurrence's h_init
  stage_rows<R>(D.zy, P.zys, b0, P.n, zin);
  dense_rows<R>(P.wy[0], P.by[0], P.zys, fy, zin, t0, true);
  dense_rows<R>(P.wy[1], P.by[1], fy, fy, t0, cat, true);
  stage_rows<R>(D.zm, D.zs, b0, P.n, zin);
  dense_rows<R>(D.w[0], D.b[0], D.zs, D.fm, zin, t0, true);
  dense_rows<R>(D.w[1], D.b[1], D.fm, D.fm, t0, cat + fy * R, true);
  if (D.y_hat) {
    dense_rows<R>(P.wy[2], P.by[2], fy, fy, cat, t0, true);
    dense_rows<R>(P.wy[3], P.by[3], fy, P.od, t0, t1, false);
    store_rows<R>(t1, D.y_hat, P.od, b0, P.n, tid);
  }
  for (int e = tid; e < h * R; e += blockDim.x) {
    const int k = e / R, r = e - k * R;
    emb[r * h + k] = cat[e];
  }
  lds_barrier();
  // the tile as a batch of its own: row r of the embedding in LDS is row r of the recurrence, and of this tile's part of hs
  SeqDev d = D.seq;
  d.h_init = emb; d.ld_init = h;
  d.hs = D.seq.hs + (int64_t)b0 * D.seq.Hp;
  const int rows = min(R, P.n - b0);
  const int64_t hs_step = (int64_t)P.n * D.seq.Hp;
  MFM_TUPLE3((small_fwd_body<KQ, R, false, false, false, true>(d, P.T, rows, 0, lds, nullptr, 0u, 0,
                                                                HoCtl{nullptr, nullptr, nullptr, 5000000ll, 1u}, hs_step)))
}

// ---------------------------------------------------------------- host
static const int kGenEnc[GEN_ENC] = {8, 2, 20, 30};      // the canonical sizes: encoders h = 32 / 8 / 80 / 120 ...
static const int kGenDec[GEN_DEC] = {26, 6, 6};          // ... decoders h = 104 / 24 / 24

// the launch(es) of one chunk of n rows (infer_launch_tuple_or_each)
template <int R>
static int encode_launch(EncodeDev& P, int threads, size_t lds_bytes, hipStream_t stream) {
  bool canon = true;
  for (int i = 0; i < GEN_ENC; ++i) canon = canon && P.d[i].seq.hk4 == kGenEnc[i];
  return infer_launch_tuple_or_each<R>("encode klef", "encode_klef_kernel", P, canon ? encode_klef_kernel<R, 8, 2, 20, 30> : nullptr,
                                       [](auto kk) { return encode_klef_kernel<R, decltype(kk)::value, 0, 0, 0>; }, threads, lds_bytes, stream);
}

template <int R>
static int decode_launch(const char* who, DecodeDev& P, int threads, size_t lds_bytes, hipStream_t stream) {
  bool canon = P.count == GEN_DEC;       // (fewer: one case of mfm_impute_missing, one LSTM -- its launch is the per-size instantiation)
  for (int i = 0; canon && i < GEN_DEC; ++i) canon = P.d[i].seq.hk4 == kGenDec[i];
  return infer_launch_tuple_or_each<R>(who, "decode_factors_kernel", P, canon ? decode_factors_kernel<R, 26, 6, 6> : nullptr,
                                       [](auto kk) { return decode_factors_kernel<R, decltype(kk)::value, 0, 0>; }, threads, lds_bytes, stream);
}

int decode_factors_launch(const char* who, DecodeDev& P, int R, int threads, size_t lds_bytes, hipStream_t stream) {
  return (R == 1) ? decode_launch<1>(who, P, threads, lds_bytes, stream) : decode_launch<4>(who, P, threads, lds_bytes, stream);
}

#define ENC_OFFS 40      // per encoder: lstm weight_ih, weight_hh, bias_ih, bias_hh, then weight and bias of fc1, mean head, logvar head

int encode_klef_prepare(const char* who, int T, int64_t N, int d_l, int d_a, int d_v, int zl, int za, int zv, int zy, const float* params,
                        const int64_t* offs, float* ws, int64_t max_rows, EncLaunch& L) {
  int rc = infer_check_rows(who, N, max_rows);
  if (rc != MFM_OK) return rc;
  if ((rc = infer_check_offsets(who, offs, ENC_OFFS, 10)) != MFM_OK) return rc;
  const int D = d_l + d_a + d_v;
  const int hh[GEN_ENC] = {zl, za, zv, zl + za + zv}, zs[GEN_ENC] = {zl, za, zv, zy};
  const int dd[GEN_ENC] = {d_l, d_a, d_v, D}, col[GEN_ENC] = {0, d_l, d_l + d_a, 0};
  const int rows = (int)gen_rows(N, max_rows);
  const int R = gen_tile_rows(GEN_ENC, rows);
  int maxw = 1, threads = 64;
  size_t lds_floats = 0;
  for (int i = 0; i < GEN_ENC; ++i) {
    if ((rc = infer_check_resident(who, hh[i])) != MFM_OK) return rc;
    maxw = std::max(maxw, std::max(hh[i], zs[i]));
    threads = std::max(threads, 8 * round_up(hh[i], 16));
  }
  for (int i = 0; i < GEN_ENC; ++i) lds_floats = std::max(lds_floats, enc_lds_floats(hh[i], R, 3, maxw));
  const size_t lds_bytes = lds_bytes_of(lds_floats);
  if ((rc = infer_check_lds(who, lds_bytes, maxw, R)) != MFM_OK) return rc;
  if ((rc = infer_check_chunk(who, rows, T, std::max(D, 4 * round_up(hh[3], 16)), "projection")) != MFM_OK) return rc;

  EncodeDev& P = L.P;
  memset(&L, 0, sizeof(L));
  float* g0 = ws;
  for (int i = 0; i < GEN_ENC; ++i) {
    EncOne& E = P.d[i];
    const int64_t* o = offs + 10 * i;
    seq_fill(E.seq, params + o[0], params + o[1], params + o[2], params + o[3], hh[i], 0);
    E.seq.gates = g0; g0 += (int64_t)rows * T * 4 * E.seq.Hp;
    for (int l = 0; l < 3; ++l) { E.w[l] = params + o[4 + 2 * l]; E.b[l] = params + o[5 + 2 * l]; }
    E.zs = zs[i];
    L.dd[i] = dd[i]; L.col[i] = col[i];
  }
  P.count = GEN_ENC; P.T = T; P.maxw = maxw;
  L.R = R; L.threads = threads; L.rows = rows; L.D = D; L.lds_bytes = lds_bytes;
  return MFM_OK;
}

int encode_klef_chunk(EncLaunch& L, const float* x, int64_t N, int64_t n0, int n, float* const* out, hipStream_t stream) {
  EncodeDev& P = L.P;
  const int T = P.T, D = L.D;
  // gates_e[t][i][g][u] = x_e[t][n0 + i] . W_ih[g h + u] + b_ih + b_hh; pad units u >= h exact zeros
  const bool whole = n == N;           // one chunk: the T * N rows of x are one matrix
  int rc = gemm_group_each(GEN_ENC * (whole ? 1 : T), stream, [&](int p, MfmGemmDesc& d) {
    const int e = p % GEN_ENC, t = p / GEN_ENC;
    const SeqDev& s = P.d[e].seq;
    xproj_desc(d, s, x + ((int64_t)t * N + n0) * D + L.col[e], D, L.dd[e], whole ? T * n : n, s.gates + (int64_t)t * n * 4 * s.Hp);
  });
  if (rc != MFM_OK) return rc;
  P.n = n;
  for (int i = 0; i < GEN_ENC; ++i) { P.d[i].mu = out[i]; P.d[i].lv = out[4 + i]; }
  return (L.R == 1) ? encode_launch<1>(P, L.threads, L.lds_bytes, stream) : encode_launch<4>(P, L.threads, L.lds_bytes, stream);
}

static int encode_klef(int T, int64_t N, int d_l, int d_a, int d_v, int zl, int za, int zv, int zy, const float* params,
                       const int64_t* offs, const float* x, float* ws, float* const* out, int64_t max_rows, hipStream_t stream) {
  static const char* who = "encode klef";
  MFM_REQUIRE(T >= 1 && N >= 1 && d_l >= 1 && d_a >= 1 && d_v >= 1 && zl >= 1 && za >= 1 && zv >= 1 && zy >= 1,
              "%s: sizes must be positive (T %d, N %lld, dims %d %d %d, z %d %d %d %d)", who, T, (long long)N, d_l, d_a, d_v, zl, za, zv, zy);
  MFM_REQUIRE(params && offs && x && ws && out, "%s: bad arguments (params, offsets, x, workspace and outputs must not be null)", who);
  for (int i = 0; i < 8; ++i) MFM_REQUIRE(out[i], "%s: output %d is null", who, i);
  int rc = infer_check_aligned(who, params, x, ws);
  if (rc != MFM_OK) return rc;
  EncLaunch L;
  if ((rc = encode_klef_prepare(who, T, N, d_l, d_a, d_v, zl, za, zv, zy, params, offs, ws, max_rows, L)) != MFM_OK) return rc;
  for (int64_t n0 = 0; n0 < N; n0 += L.rows) {
    const int n = (int)std::min<int64_t>(L.rows, N - n0);
    float* o[2 * GEN_ENC];
    for (int i = 0; i < GEN_ENC; ++i) { o[i] = out[i] + n0 * L.P.d[i].zs; o[4 + i] = out[4 + i] + n0 * L.P.d[i].zs; }
    if ((rc = encode_klef_chunk(L, x, N, n0, n, o, stream)) != MFM_OK) return rc;
  }
  return MFM_OK;
}

#define DEC_OFFS 38      // weight, bias of zy_to_fy fc1, fc2, zl_to_fl .., za_to_fa .., zv_to_fv ..; 3 x (lstm weight_ih, weight_hh,
                         // bias_ih, bias_hh, fc1 weight, bias); weight, bias of fy_to_y fc1, fc2

int decode_factors_prepare(const char* who, int T, int64_t N, const int32_t* sz, const float* params, const int64_t* offs, float* ws,
                           int64_t max_rows, DecLaunch& L) {
  int rc = infer_check_rows(who, N, max_rows);
  if (rc != MFM_OK) return rc;
  if ((rc = infer_check_offsets(who, offs, DEC_OFFS, 6, 16, 34)) != MFM_OK) return rc;
  const int zs[GEN_DEC] = {sz[0], sz[1], sz[2]}, zys = sz[3], fm[GEN_DEC] = {sz[4], sz[5], sz[6]}, fy = sz[7];
  const int dm[GEN_DEC] = {sz[8], sz[9], sz[10]}, od = sz[11];
  const int rows = (int)gen_rows(N, max_rows);
  const int R = gen_tile_rows(GEN_DEC, rows);
  int maxw = std::max(std::max(zys, fy), od), threads = 64;
  size_t seq_floats = 0;
  for (int i = 0; i < GEN_DEC; ++i) {
    const int h = fy + fm[i];
    if ((rc = infer_check_resident(who, h)) != MFM_OK) return rc;
    maxw = std::max(maxw, std::max(h, zs[i]));
    threads = std::max(threads, 8 * round_up(h, 16));
    seq_floats = std::max(seq_floats, seq_lds_floats(h, R));
  }
  const size_t lds_bytes = lds_bytes_of(seq_floats + (size_t)5 * maxw * R);
  if ((rc = infer_check_lds(who, lds_bytes, maxw, R)) != MFM_OK) return rc;
  if ((rc = infer_check_chunk(who, rows, T, std::max(round_up(maxw, 16), std::max(dm[0], std::max(dm[1], dm[2]))), "product")) != MFM_OK) return rc;

  DecodeDev& P = L.P;
  memset(&L, 0, sizeof(L));
  float* h0 = ws;
  for (int i = 0; i < GEN_DEC; ++i) {
    DecOne& Dd = P.d[i];
    const int64_t* o = offs + 16 + 6 * i;
    seq_fill(Dd.seq, params + o[0], params + o[1], params + o[2], params + o[3], fy + fm[i], 1);
    L.fcw[i] = params + o[4]; L.fcb[i] = params + o[5];
    Dd.seq.hs = h0; h0 += (int64_t)rows * T * Dd.seq.Hp;
    for (int l = 0; l < 2; ++l) { Dd.w[l] = params + offs[4 + 4 * i + 2 * l]; Dd.b[l] = params + offs[5 + 4 * i + 2 * l]; }
    Dd.zs = zs[i]; Dd.fm = fm[i];
    L.dm[i] = dm[i];
  }
  for (int l = 0; l < 2; ++l) {
    P.wy[l] = params + offs[2 * l]; P.by[l] = params + offs[2 * l + 1];
    P.wy[2 + l] = params + offs[34 + 2 * l]; P.by[2 + l] = params + offs[35 + 2 * l];
  }
  P.count = GEN_DEC; P.T = T; P.zys = zys; P.fy = fy; P.od = od; P.maxw = maxw; P.seq_floats = (int)seq_floats;
  L.R = R; L.threads = threads; L.rows = rows; L.lds_bytes = lds_bytes;
  return MFM_OK;
}

int decode_factors_chunk(const char* who, DecLaunch& L, const float* const* z, float* y_hat, int n, hipStream_t stream) {
  DecodeDev& P = L.P;
  P.n = n;
  // the three decoders share the one zy; decoder l's workgroups write y_hat
  for (int i = 0; i < GEN_DEC; ++i) { P.d[i].zm = z[i]; P.d[i].zy = z[3]; }
  P.d[0].y_hat = y_hat;
  return decode_factors_launch(who, P, L.R, L.threads, L.lds_bytes, stream);
}

static int decode_factors(int T, int64_t N, const int32_t* sz, const float* params, const int64_t* offs, const float* const* z,
                          float* ws, float* const* out, int64_t max_rows, hipStream_t stream) {
  static const char* who = "decode factors";
  MFM_REQUIRE(sz && params && offs && z && ws && out, "%s: bad arguments (sizes, params, offsets, factors, workspace and outputs must not be null)", who);
  int rc = infer_check_sizes(who, T, N, sz);
  if (rc != MFM_OK) return rc;
  for (int i = 0; i < 4; ++i) MFM_REQUIRE(z[i] && out[i], "%s: factor / output %d is null", who, i);
  MFM_REQUIRE((((uintptr_t)params | (uintptr_t)ws) & 15) == 0, "%s: params and workspace must be 16-byte aligned", who);
  DecLaunch L;
  if ((rc = decode_factors_prepare(who, T, N, sz, params, offs, ws, max_rows, L)) != MFM_OK) return rc;
  const DecodeDev& P = L.P;
  for (int64_t n0 = 0; n0 < N; n0 += L.rows) {
    const int n = (int)std::min<int64_t>(L.rows, N - n0);
    const float* zc[4] = {z[0] + n0 * sz[0], z[1] + n0 * sz[1], z[2] + n0 * sz[2], z[3] + n0 * sz[3]};
    if ((rc = decode_factors_chunk(who, L, zc, out[3] + n0 * sz[11], n, stream)) != MFM_OK) return rc;
    // x_hat_m[t][n0 + i] = hs_m[t][i] . Wfc_m^T + b
    const bool whole = n == N;
    rc = gemm_group_each(GEN_DEC * (whole ? 1 : T), stream, [&](int p, MfmGemmDesc& d) {
      const int m = p % GEN_DEC, t = p / GEN_DEC;
      const SeqDev& s = P.d[m].seq;
      dec_fc1_desc(d, s, s.hs + (int64_t)t * n * s.Hp, L.fcw[m], L.fcb[m], out[m] + ((int64_t)t * N + n0) * L.dm[m], L.dm[m], whole ? T * n : n);
    });
    if (rc != MFM_OK) return rc;
  }
  return MFM_OK;
}

}  // namespace mfm

extern "C" int64_t mfm_encode_klef_workspace_floats(int32_t T, int64_t N, int32_t zl, int32_t za, int32_t zv, int64_t max_rows) {
  if (T < 1 || N < 1 || zl < 1 || za < 1 || zv < 1 || max_rows < 0) return 0;
  return mfm::encode_ws_floats(T, N, zl, za, zv, max_rows);
}

extern "C" int mfm_encode_klef(int32_t T, int64_t N, int32_t d_l, int32_t d_a, int32_t d_v, int32_t zl, int32_t za, int32_t zv,
                               int32_t zy, const float* params, const int64_t* offsets, const float* x, float* workspace,
                               float* const* out, int64_t max_rows, void* stream) {
  return mfm::encode_klef(T, N, d_l, d_a, d_v, zl, za, zv, zy, params, offsets, x, workspace, out, max_rows, (hipStream_t)stream);
}

extern "C" int64_t mfm_decode_factors_workspace_floats(int32_t T, int64_t N, int32_t fy, int32_t fl, int32_t fa, int32_t fv,
                                                       int64_t max_rows) {
  if (T < 1 || N < 1 || fy < 1 || fl < 1 || fa < 1 || fv < 1 || max_rows < 0) return 0;
  return mfm::decode_ws_floats(T, N, fy, fl, fa, fv, max_rows);
}

extern "C" int mfm_decode_factors(int32_t T, int64_t N, const int32_t* sizes, const float* params, const int64_t* offsets,
                                  const float* const* z, float* workspace, float* const* out, int64_t max_rows, void* stream) {
  return mfm::decode_factors(T, N, sizes, params, offsets, z, workspace, out, max_rows, (hipStream_t)stream);
}
