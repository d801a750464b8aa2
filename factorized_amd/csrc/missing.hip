// The missing-modality test protocol (include/mfm_hip.h, mfm_predict_missing): what the `predict` / `score` blocks of the
// reference's train_mfm_missing, seq2seq and basic_missing loops report per missing case m -- the error of the rebuilt modality,
// the label prediction and its label loss -- on what those numbers depend on alone, for the three classes of the family:
//   family 0, MFM_missing    y_hat_m = decoded_no<m>[3], gen_m = mse(decoded_no<m>[index of m], x_m), disc_m = label loss of y_hat_m
//   family 1, seq2seq        gen_m = mse(decoder_m(relu(fc2(relu(fc1(encoder_<pair>_to_<m>(pair))))), T), x_m); no label path
//   family 2, basic_missing  y_hat_m = zy_no<m>_to_y_fc2(relu(zy_no<m>_to_y_fc1(encoder_<pair>_to_y(pair)))), disc_m; no decoder
// No reconstruction is written: the decoders' fc1 is fused with the squared error against x_m.  Per row chunk and for the cases
// asked for (one of l / a / v, or all three), on one stream:
//   0. + 1. the gather of the observed pairs and the grouped x-projection GEMM of mfm_impute_missing (impute.hip): x is read by
//      the gather (the observed columns) and by step 4 (the missing modality's columns, as the target) alone;
//   2. the encoder recurrences.  Families 0 and 1: impute_encode_kernel (impute.hip), the encoders -> z_m and (family 0) -> zy;
//      family 2: missing_label_kernel, workgroup (case, row tile) runs the T-step recurrence, the encoder's fc1 on the last hidden
//      state still in LDS and the case's own two-layer head, and writes y_hat: zy never leaves the chip;
//   3. the decoder recurrences storing h_t alone.  Family 0: decode_factors_kernel as mfm_impute_missing launches it (generate.hip);
//      family 1: decode_plain_kernel, the same without the fy half -- workgroup (case, row tile) stages its rows of z_m, applies
//      the two dense layers into LDS, transposes the embedding and runs the decoder form of the recurrence with h = f_m;
//   4. fc1_sqerr_kernel (objective.hip) over the stored h of the cases' decoders against the missing modality's columns of x:
//      one partial per workgroup;
//   5. zeros_finish_kernel (zeros.hip), one workgroup: the chunk's partials and its label-loss sums in a fixed order in fp64 into
//      six accumulators of the workspace; behind the last chunk gen and disc, divided by the counts of the WHOLE split.
// No float atomics: the results are bit-identical from run to run for a given (T, N, max_rows).  Launches 2 and 3 follow the launch
// rules of infer_dev.h: the per-block switch for the canonical size tuple only, else one launch per LSTM.
#include "infer_dev.h"

namespace mfm {

#define MIS_FAMILIES 3

struct MisHead {
  SeqDev seq;                                  // gates (the x-projections, read only), w_hh, h = zy, Hp, hk4
  const float* w[3]; const float* b[3];        // the encoder's fc1, zy_no<m>_to_y fc1, fc2
  float* y_hat;                                // this chunk's rows [n, od]
  int block_begin;
};
struct MisLabelDev { MisHead d[IMP_CASES]; int count, T, n, maxw, fy, od; };

template <int R, int K0, int K1, int K2>
__global__ __launch_bounds__(1024) void missing_label_kernel(const MisLabelDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, bid = blockIdx.x;
  MFM_SEQ_BLOCK_LSTM(P, bid, di)
  const MisHead& E = P.d[di];
  const int tile = bid - E.block_begin, b0 = tile * R;
  const float* hT = nullptr;
  MFM_TUPLE3(hT = small_fwd_body<KQ, R, false, false, false>(E.seq, P.T, P.n, tile, lds))
  // the two h buffers stay where they are; two activations behind them ([maxw][R] each): zy and y_hat in the first, the head's
  // hidden layer in the second
  float* act0 = lds + 2 * E.seq.Hp * R;
  float* act1 = act0 + P.maxw * R;
  const int h = E.seq.h;
  dense_rows<R>(E.w[0], E.b[0], h, h, hT, act0, false);
  dense_rows<R>(E.w[1], E.b[1], h, P.fy, act0, act1, true);
  dense_rows<R>(E.w[2], E.b[2], P.fy, P.od, act1, act0, false);
  store_rows<R>(act0, E.y_hat, P.od, b0, P.n, tid);
}

// decode_factors_kernel (generate.hip) without its fy half: the embedding is f_m alone, no classifier.  Of P: d[.].seq / w / b /
// zm / zs / fm, count, T, n, maxw, seq_floats
template <int R, int K0, int K1, int K2>
__global__ __launch_bounds__(1024) void decode_plain_kernel(const DecodeDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, bid = blockIdx.x;
  MFM_SEQ_BLOCK_LSTM(P, bid, di)
  const DecOne& D = P.d[di];
  const int tile = bid - D.block_begin, b0 = tile * R;
  const int h = D.seq.h;
  // behind everything the recurrence uses: the embedding must survive its weight staging
  float* zin = lds + P.seq_floats;             // [maxw][R] each
  float* t0 = zin + P.maxw * R;
  float* cat = t0 + P.maxw * R;                // f_m as [h][R]
  float* emb = cat + P.maxw * R;               // the same as [R][h]: the recurrence's h_init
  stage_rows<R>(D.zm, D.zs, b0, P.n, zin);
  dense_rows<R>(D.w[0], D.b[0], D.zs, D.fm, zin, t0, true);
  dense_rows<R>(D.w[1], D.b[1], D.fm, D.fm, t0, cat, true);
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
static const int kMisLabel[IMP_CASES] = {8, 8, 8};        // the canonical sizes: the encoders -> zy h = 32 ...
static const int kMisDec[IMP_CASES] = {22, 2, 2};         // ... the decoders of seq2seq h = fl / fa / fv = 88 / 8 / 8

template <int R>
static int mis_label_launch(const char* who, MisLabelDev& P, int threads, size_t lds_bytes, hipStream_t stream) {
  bool canon = P.count == IMP_CASES;       // (one case: one LSTM -- its launch is the per-size instantiation)
  for (int i = 0; canon && i < IMP_CASES; ++i) canon = P.d[i].seq.hk4 == kMisLabel[i];
  return infer_launch_tuple_or_each<R>(who, "missing_label_kernel", P, canon ? missing_label_kernel<R, 8, 8, 8> : nullptr,
                                       [](auto kk) { return missing_label_kernel<R, decltype(kk)::value, 0, 0>; }, threads, lds_bytes, stream);
}

template <int R>
static int mis_decode_launch(const char* who, DecodeDev& P, int threads, size_t lds_bytes, hipStream_t stream) {
  bool canon = P.count == IMP_CASES;
  for (int i = 0; canon && i < IMP_CASES; ++i) canon = P.d[i].seq.hk4 == kMisDec[i];
  return infer_launch_tuple_or_each<R>(who, "decode_plain_kernel", P, canon ? decode_plain_kernel<R, 22, 2, 2> : nullptr,
                                       [](auto kk) { return decode_plain_kernel<R, decltype(kk)::value, 0, 0>; }, threads, lds_bytes, stream);
}

// workgroups (= partial slots) of fc1_sqerr_kernel over a chunk of n rows, the decoders of the cases asked for alone
static int64_t mis_sq_tiles(int64_t T, int64_t n, const ImpSizes& S) {
  int64_t t = 0;
  for (int c = 0; c < S.nc; ++c) t += ((T * n + OBJ_BM - 1) / OBJ_BM) * ((S.dm[S.cs[c]] + OBJ_BN - 1) / OBJ_BN);
  return t;
}

// the hidden size of case m's decoder: [fy | f_m] (family 0), f_m (family 1)
static int mis_dec_h(const ImpSizes& S, int family, int m) { return (family == 0 ? S.fy : 0) + S.fm[m]; }

// the workspace, in this order (every part a multiple of 4 floats): per case asked for what its launches of one chunk need -- the
// x-projections of its encoder -> z_m (families 0, 1) and -> zy (0, 2), its z_m (0, 1) and zy (0) rows, its decoder's stored h
// (0, 1), its gathered pair; then the squared-error partials (0, 1), the ZER_ACC fp64 accumulators, and 4 floats that take the
// finish's gen where the family has none
struct MisLayout { int64_t part, acc, gen, total; };
static MisLayout mis_layout(int64_t T, int64_t N, const ImpSizes& S, int family, int64_t max_rows) {
  const int64_t rows = gen_rows(N, max_rows);
  int64_t f = 0;
  for (int c = 0; c < S.nc; ++c) {
    const int m = S.cs[c];
    f += rows * T * S.ld[m];
    if (family != 2) f += rows * T * 4 * hp_of(S.z[m]) + up4(rows * S.z[m]) + rows * T * hp_of(mis_dec_h(S, family, m));
    if (family != 1) f += rows * T * 4 * hp_of(S.zy);
    if (family == 0) f += up4(rows * S.zy);
  }
  MisLayout o;
  o.part = f;
  o.acc = o.part + (family != 2 ? up4(mis_sq_tiles(T, rows, S)) : 0);
  o.gen = o.acc + up4(2 * ZER_ACC);
  o.total = o.gen + 4;
  return o;
}

// rows per workgroup of the encoders' launch and of the decoders' (0: the family has none)
static void mis_tile_rows(int family, int nc, int rows, int* Re, int* Rd) {
  *Re = gen_tile_rows(family == 0 ? 2 * nc : nc, rows);
  *Rd = family == 2 ? 0 : gen_tile_rows(nc, rows);
}

// which of a case's IMP_CASE_PTRS parameter slots a family reads
static bool mis_slot_used(int family, int i) {
  if (family == 0) return true;
  if (family == 1) return i < 6 || i >= 12;
  return i >= 6 && i < 16;
}

static int predict_missing(int T, int64_t N, const int32_t* sz, int family, int cases, int loss_kind, const float* const* prm,
                           const float* x, const void* y, float* ws, float* y_hat, float* gen, float* disc, int64_t max_rows,
                           hipStream_t stream) {
  static const char* who = "predict missing";
  MFM_REQUIRE(sz && prm && x && ws, "%s: bad arguments (sizes, parameter table, x and workspace must not be null)", who);
  MFM_REQUIRE(family >= 0 && family < MIS_FAMILIES, "%s: family = %d (0 MFM_missing, 1 seq2seq, 2 basic_missing)", who, family);
  int rc = infer_check_sizes(who, T, N, sz);
  if (rc != MFM_OK) return rc;
  MFM_REQUIRE(cases == 1 || cases == 2 || cases == 4 || cases == 7, "%s: cases = %d (bit 0 l, bit 1 a, bit 2 v: one of them, or all three)", who, cases);
  if ((rc = infer_check_loss_kind(who, loss_kind)) != MFM_OK) return rc;
  if ((rc = infer_check_rows(who, N, max_rows)) != MFM_OK) return rc;
  const bool has_gen = family != 2, has_label = family != 1;
  MFM_REQUIRE(!has_gen || gen, "%s: gen must not be null for family %d", who, family);
  MFM_REQUIRE(!has_label || y_hat, "%s: y_hat must not be null for family %d", who, family);
  MFM_REQUIRE(!has_label || (y != nullptr) == (disc != nullptr), "%s: labels and disc come together (both, or both null)", who);
  if (!has_label) { y = nullptr; disc = nullptr; y_hat = nullptr; }
  // (x is read element by element: by the gather, and as the squared error's target; the GEMMs and the recurrences read the
  // workspace 16 bytes at a time)
  MFM_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)ws & 15) == 0, "%s: x must be 4-byte aligned, the workspace 16-byte aligned", who);
  MFM_REQUIRE((((uintptr_t)y_hat | (uintptr_t)gen | (uintptr_t)disc) & 3) == 0 && ((uintptr_t)y & (loss_kind == 0 ? 3 : 7)) == 0,
              "%s: y_hat, gen, disc or the labels are misaligned", who);
  ImpSizes S;
  imp_sizes(sz, cases, S);
  for (int c = 0; c < S.nc; ++c) {
    const int m = S.cs[c];
    for (int i = 0; i < IMP_CASE_PTRS; ++i) {
      if (!mis_slot_used(family, i)) continue;
      const float* p = prm[m * IMP_CASE_PTRS + i];
      MFM_REQUIRE(p, "%s: parameter %d of case %d is null", who, i, m);
      const bool lstm_w = i == 0 || i == 1 || i == 6 || i == 7 || i == 16 || i == 17;
      MFM_REQUIRE(((uintptr_t)p & (lstm_w ? 15 : 3)) == 0, "%s: parameter %d of case %d is misaligned (LSTM weights 16 bytes, the rest 4)", who, i, m);
    }
  }
  for (int i = IMP_CASES * IMP_CASE_PTRS; family == 0 && i < IMP_NPARAM; ++i)
    MFM_REQUIRE(prm[i] && ((uintptr_t)prm[i] & 3) == 0, "%s: shared parameter %d is null or misaligned", who, i - IMP_CASES * IMP_CASE_PTRS);

  const int rows = (int)gen_rows(N, max_rows);
  int Re, Rd;
  mis_tile_rows(family, S.nc, rows, &Re, &Rd);
  int enc_maxw = family == 2 ? std::max(S.fy, S.od) : 1, enc_threads = 64, dec_threads = 64, maxd = 1, maxhp = 16;
  int dec_maxw = family == 0 ? std::max(std::max(S.zy, S.fy), S.od) : 1;
  size_t enc_floats = 0, dec_seq = 0;
  for (int c = 0; c < S.nc; ++c) {
    const int m = S.cs[c];
    // the encoder -> z_m, the encoder -> zy, the decoder (0: the family has no such LSTM)
    const int hs[3] = {has_gen ? S.z[m] : 0, has_label ? S.zy : 0, has_gen ? mis_dec_h(S, family, m) : 0};
    for (int i = 0; i < 3; ++i)
      if (hs[i] && (rc = infer_check_resident(who, hs[i])) != MFM_OK) return rc;
    enc_maxw = std::max(enc_maxw, std::max(hs[0], hs[1]));
    enc_threads = std::max(enc_threads, 8 * round_up(std::max(hs[0], hs[1]), 16));
    if (has_gen) {
      dec_maxw = std::max(dec_maxw, std::max(hs[2], std::max(S.z[m], S.fm[m])));
      dec_threads = std::max(dec_threads, 8 * round_up(hs[2], 16));
      dec_seq = std::max(dec_seq, seq_lds_floats(hs[2], Rd));
    }
    maxd = std::max(maxd, std::max(S.dm[m], S.ld[m]));
    maxhp = std::max(maxhp, round_up(std::max(std::max(hs[0], hs[1]), hs[2]), 16));
  }
  // the layout rule of the LDS: an encoder workgroup keeps the two h buffers and puts its activations [maxw][R] behind them (one
  // of impute_encode_kernel, two of missing_label_kernel); a decoder workgroup puts its [maxw][R] buffers (five of
  // decode_factors_kernel, four of decode_plain_kernel) behind everything the recurrence lays out
  for (int c = 0; c < S.nc; ++c) {
    if (has_gen) enc_floats = std::max(enc_floats, enc_lds_floats(S.z[S.cs[c]], Re, 1, enc_maxw));
    if (has_label) enc_floats = std::max(enc_floats, enc_lds_floats(S.zy, Re, family == 2 ? 2 : 1, enc_maxw));
  }
  const size_t enc_lds = lds_bytes_of(enc_floats);
  const size_t dec_lds = has_gen ? lds_bytes_of(dec_seq + (size_t)(family == 0 ? 5 : 4) * dec_maxw * Rd) : 0;
  if ((rc = infer_check_lds(who, std::max(enc_lds, dec_lds), std::max(enc_maxw, dec_maxw), enc_lds > dec_lds ? Re : Rd)) != MFM_OK) return rc;
  if ((rc = infer_check_chunk(who, rows, T, std::max(std::max(S.D, maxd), 4 * maxhp), "product")) != MFM_OK) return rc;
  MFM_REQUIRE(mis_sq_tiles(T, rows, S) < ((int64_t)1 << 31), "%s: a chunk of %d rows x %d steps is too large; pass a row cap", who, rows, T);

  const MisLayout lay = mis_layout(T, N, S, family, max_rows);
  ImpEncodeDev PE;
  DecodeDev PD;
  MisLabelDev PL;
  Fc1SqLaunch Sq;
  ImpGather G;
  memset(&PE, 0, sizeof(PE));
  memset(&PD, 0, sizeof(PD));
  memset(&PL, 0, sizeof(PL));
  memset(&Sq, 0, sizeof(Sq));
  memset(&G, 0, sizeof(G));
  G.x = x; G.N = N; G.T = T; G.D = S.D;
  SeqDev* enc_seq[IMP_ENC];                    // the LSTMs of the projection GEMM, and the case slot of each
  int enc_slot[IMP_ENC], nenc = 0;
  float* zbuf[IMP_CASES][2] = {};
  Sq.hmax = 1;
  float* w0 = ws;
  for (int c = 0; c < S.nc; ++c) {
    const int m = S.cs[c];
    const float* const* p = prm + m * IMP_CASE_PTRS;
    if (has_gen) {
      ImpEnc& E = PE.d[PE.count++];
      seq_fill(E.seq, p[0], p[1], p[2], p[3], S.z[m], 0);
      E.w = p[4]; E.b = p[5];
      enc_seq[nenc] = &E.seq; enc_slot[nenc++] = c;
    }
    if (family == 0) {
      ImpEnc& E = PE.d[PE.count++];
      seq_fill(E.seq, p[6], p[7], p[8], p[9], S.zy, 0);
      E.w = p[10]; E.b = p[11];
      enc_seq[nenc] = &E.seq; enc_slot[nenc++] = c;
    }
    if (family == 2) {
      MisHead& H = PL.d[PL.count++];
      seq_fill(H.seq, p[6], p[7], p[8], p[9], S.zy, 0);
      for (int l = 0; l < 3; ++l) { H.w[l] = p[10 + 2 * l]; H.b[l] = p[11 + 2 * l]; }
      enc_seq[nenc] = &H.seq; enc_slot[nenc++] = c;
    }
    for (int e = nenc - (family == 0 ? 2 : 1); e < nenc; ++e) { enc_seq[e]->gates = w0; w0 += (int64_t)rows * T * 4 * enc_seq[e]->Hp; }
    if (has_gen) { zbuf[c][0] = w0; w0 += up4((int64_t)rows * S.z[m]); }
    if (family == 0) { zbuf[c][1] = w0; w0 += up4((int64_t)rows * S.zy); }
    if (has_gen) {
      DecOne& Dd = PD.d[c];
      seq_fill(Dd.seq, p[16], p[17], p[18], p[19], mis_dec_h(S, family, m), 1);
      Dd.seq.hs = w0; w0 += (int64_t)rows * T * Dd.seq.Hp;
      for (int l = 0; l < 2; ++l) { Dd.w[l] = p[12 + 2 * l]; Dd.b[l] = p[13 + 2 * l]; }
      Dd.zs = S.z[m]; Dd.fm = S.fm[m];
      Fc1SqItem& I = Sq.F.it[m];
      I.hs = Dd.seq.hs; I.w = p[20]; I.bias = p[21];
      I.d = S.dm[m]; I.h = Dd.seq.h; I.Hp = Dd.seq.Hp; I.col_tiles = cdiv(S.dm[m], OBJ_BN);
      Sq.hmax = std::max(Sq.hmax, Dd.seq.h);
    }
    imp_gather_case(G, c, m, S, w0); w0 += (int64_t)rows * T * S.ld[m];
  }
  // (the items of the cases not asked for keep col_tiles 0: no workgroup, no partial)
  for (int m = 0; m < IMP_CASES; ++m) {
    Sq.col[m] = m == 0 ? 0 : Sq.col[m - 1] + S.dm[m - 1];
    Sq.inv_gen[m] = 1.0 / ((double)T * (double)N * (double)S.dm[m]);
  }
  Sq.F.D = S.D; Sq.F.N = N; Sq.T = T;
  if (family == 0)
    for (int l = 0; l < 4; ++l) { PD.wy[l] = prm[IMP_CASES * IMP_CASE_PTRS + 2 * l]; PD.by[l] = prm[IMP_CASES * IMP_CASE_PTRS + 2 * l + 1]; }
  PE.T = T; PE.maxw = enc_maxw;
  PL.T = T; PL.maxw = enc_maxw; PL.fy = S.fy; PL.od = S.od;
  PD.count = has_gen ? S.nc : 0; PD.T = T; PD.od = S.od; PD.maxw = dec_maxw; PD.seq_floats = (int)dec_seq;
  if (family == 0) { PD.zys = S.zy; PD.fy = S.fy; }

  ZerFinishDev Q;
  memset(&Q, 0, sizeof(Q));
  for (int m = 0; m < IMP_CASES; ++m) Q.inv_gen[m] = Sq.inv_gen[m];
  Q.acc = reinterpret_cast<double*>(ws + lay.acc);      // (a multiple of 4 floats from a 16-byte aligned base)
  Q.gen = has_gen ? gen : ws + lay.gen;
  Q.disc = disc;
  Q.inv_disc = inv_label_count(loss_kind, N, S.od);
  Q.od = S.od; Q.loss_kind = loss_kind;
  float* part = ws + lay.part;

  for (int64_t n0 = 0; n0 < N; n0 += rows) {
    const int n = (int)std::min<int64_t>(rows, N - n0);
    G.n0 = n0; G.n = n;
    if ((rc = impute_gather_launch(G, S.nc, stream)) != MFM_OK) return rc;
    // gates_e[t][i][g][u] = pair_e[t][i] . W_ih[g h + u] + b_ih + b_hh; pad units u >= h exact zeros.  The gathered pair of a
    // chunk is one [T * n, ld] matrix whatever the chunk
    rc = gemm_group_each(nenc, stream, [&](int e, MfmGemmDesc& d) {
      const int c = enc_slot[e];
      xproj_desc(d, *enc_seq[e], G.out[c], G.ld[c], G.k[c], T * n, enc_seq[e]->gates);
    });
    if (rc != MFM_OK) return rc;
    // case m's rows of y_hat: [3, N, od] for all three cases, [N, od] for one
    float* yc[IMP_CASES] = {};
    for (int c = 0; c < S.nc; ++c)
      if (has_label) yc[c] = y_hat + ((int64_t)(S.nc == IMP_CASES ? c : 0) * N + n0) * S.od;
    if (family == 2) {
      PL.n = n;
      for (int c = 0; c < S.nc; ++c) PL.d[c].y_hat = yc[c];
      rc = (Re == 1) ? mis_label_launch<1>(who, PL, enc_threads, enc_lds, stream) : mis_label_launch<4>(who, PL, enc_threads, enc_lds, stream);
      if (rc != MFM_OK) return rc;
      if (!y) continue;                        // (no squared error, no label loss: nothing to finish)
    } else {
      PE.n = PD.n = n;
      for (int c = 0; c < S.nc; ++c) {
        const int e = family == 0 ? 2 * c : c;
        PE.d[e].z = zbuf[c][0];
        if (family == 0) PE.d[e + 1].z = zbuf[c][1];
        PD.d[c].zm = zbuf[c][0]; PD.d[c].zy = zbuf[c][1];
        PD.d[c].y_hat = yc[c];
      }
      if ((rc = impute_encode_launch(who, PE, family == 0, S.cs[0], Re, enc_threads, enc_lds, stream)) != MFM_OK) return rc;
      if (family == 0) rc = decode_factors_launch(who, PD, Rd, dec_threads, dec_lds, stream);
      else rc = (Rd == 1) ? mis_decode_launch<1>(who, PD, dec_threads, dec_lds, stream) : mis_decode_launch<4>(who, PD, dec_threads, dec_lds, stream);
      if (rc != MFM_OK) return rc;
      if ((rc = fc1_sqerr_chunk(Sq, x, n0, n, part, Q.part, Q.npart, stream)) != MFM_OK) return rc;
    }
    // the finish walks three cases: those not asked for repeat the first one's y_hat (their sums go nowhere the caller reads)
    for (int m = 0; m < IMP_CASES; ++m) Q.y_hat[m] = yc[0];
    for (int c = 0; c < S.nc; ++c) Q.y_hat[S.cs[c]] = yc[c];
    Q.y = labels_at(y, loss_kind, n0, S.od);
    Q.n = n; Q.first = n0 == 0; Q.last = n0 + n == N;
    if ((rc = zeros_finish_launch(Q, stream)) != MFM_OK) return rc;
  }
  return MFM_OK;
}

}  // namespace mfm

extern "C" int64_t mfm_predict_missing_workspace_floats(int32_t T, int64_t N, const int32_t* sizes, int32_t family, int32_t cases,
                                                        int32_t with_labels, int64_t max_rows) {
  mfm::ImpSizes S;
  if (T < 1 || N < 1 || !sizes || family < 0 || family >= MIS_FAMILIES || max_rows < 0 || !mfm::imp_sizes(sizes, cases, S)) return 0;
  (void)with_labels;                           // (the label loss reads y_hat where it lies: no floats of its own)
  return mfm::mis_layout(T, N, S, family, max_rows).total;
}

extern "C" int mfm_predict_missing_tile_rows(int64_t N, int32_t family, int32_t cases, int64_t max_rows, int32_t* tile_rows) {
  if (N < 1 || max_rows < 0 || !tile_rows || family < 0 || family >= MIS_FAMILIES || (cases != 1 && cases != 2 && cases != 4 && cases != 7)) {
    mfm::set_error("predict missing tile rows: bad arguments (N %lld, family %d, cases %d, row cap %lld)", (long long)N, family, cases,
                   (long long)max_rows);
    return MFM_ERR_ARG;
  }
  const int nc = cases == 7 ? 3 : 1, rows = (int)std::min<int64_t>(mfm::gen_rows(N, max_rows), INT32_MAX);
  int Re, Rd;
  mfm::mis_tile_rows(family, nc, rows, &Re, &Rd);
  tile_rows[0] = Re; tile_rows[1] = Rd;
  return MFM_OK;
}

extern "C" int mfm_predict_missing(int32_t T, int64_t N, const int32_t* sizes, int32_t family, int32_t cases, int32_t loss_kind,
                                   const float* const* params, const float* x, const void* y, float* workspace, float* y_hat,
                                   float* gen, float* disc, int64_t max_rows, void* stream) {
  return mfm::predict_missing(T, N, sizes, family, cases, loss_kind, params, x, y, workspace, y_hat, gen, disc, max_rows,
                              (hipStream_t)stream);
}
