// The zeroed-modality test protocol of MFM_KL_EF (include/mfm_hip.h, mfm_predict_zeros_klef): what `predict(model, X_test)` of the
// reference's train_mfm_test_zeros does (mfm_mosi.py:572-596) -- the test split through the eval forward three times, each time
// with one modality's columns set to zero (cases: no l, no a, no v); y_hat of every case, and F.mse_loss of the ZEROED modality's
// reconstruction against the real x_c -- on what those results depend on alone (mfm_model.py:619-660):
//   y_hat_c   <- zy_c = last_to_zy_fc1(ef_encoder(x with modality c's columns zero)) -> fy -> the classifier
//   x_c_hat_c <- decoder_c([fy_c | f_c]) with f_c from z_c^0 = last_to_z{c}_fc1(encoder_c(zeros)): the same row for every sample
// The encoders of the two PRESENT modalities reach neither (their factors feed the other two decoders and the KLD, which the
// protocol does not look at): they do not run.  No x is copied or zeroed, no x_hat is written, no log-variance head, no KLD.
// Per row chunk, on one stream:
//   1. the ef encoder's input projection split by modality, P_m = x_m W_ih[:, columns of m]^T for m = l, a, v, as ONE grouped
//      fp32 GEMM (no bias; a chunk that is not the whole split: one problem per modality and time step): every column of x
//      meets W_ih once for the three cases;
//   2. zeros_gates_kernel: gates_c = sum over m != c of P_m, + b_ih + b_hh, for the three cases in one pass (P read once, 16
//      bytes per lane); in the first chunk it also fills the gates of the three zeroed encoders, b_ih + b_hh at every step;
//   3. zeros_encode_kernel, ONE launch: workgroup (ef encoder, case c, row tile) runs the T-step recurrence on gates_c and then
//      the encoder's fc1 and last_to_zy_fc1 -> zy_c; in the first chunk three more one-row workgroups run encoder_l / a / v on
//      the constant gates, fc1 and the mean head, and write z_c^0 once per row of a chunk (decode_factors_kernel stages its z
//      rows without a stride);
//   4. decode_factors_kernel as mfm_impute_missing launches it (generate.hip): decoder c on zy_c and z_c^0, h_t stored; every
//      decoder's workgroups run the classifier on their own fy -> y_hat_c;
//   5. fc1_sqerr_kernel (objective.hip): decoder c's fc1 fused with the squared error against the REAL x_c;
//   6. zeros_finish_kernel, one workgroup: the chunk's squared-error partials per modality and its label-loss sum per case in a
//      fixed order in fp64 into six accumulators of the workspace -- the first chunk stores, the others add, in stream order;
//      behind the last chunk it divides by the counts of the WHOLE split.
// No float atomics: the results are bit-identical from run to run for a given (T, N, max_rows).  Launch 3 follows the launch rules
// of infer_dev.h: the per-block switch for the canonical size tuple only, else one launch per LSTM.
#include "infer_dev.h"

namespace mfm {

#define ZER_LSTMS (2 * ZER_CASES)      // the ef encoder once per case, then the three zeroed encoders

struct ZerOne {
  SeqDev seq;                                  // gates (read only), w_hh, h, Hp, hk4
  const float* w[2]; const float* b[2];        // fc1, the mean head
  float* z;                                    // rep == 0: this chunk's rows [n, zs]; else [rep, zs], every row the one result
  int zs, n, rep, slot, block_begin;           // n: rows of this LSTM (1 for a zeroed encoder); slot: which of K0 .. K3 is its size
};
struct ZerEncDev { ZerOne d[ZER_LSTMS]; int count, T, maxw; };

template <int R, int K0, int K1, int K2, int K3>
__global__ __launch_bounds__(1024) void zeros_encode_kernel(const ZerEncDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, bid = blockIdx.x;
  MFM_SEQ_BLOCK_LSTM(P, bid, li)
  const ZerOne& E = P.d[li];
  const int di = E.slot;
  const int tile = bid - E.block_begin, b0 = tile * R;
  const float* hT = nullptr;
  MFM_TUPLE4(hT = small_fwd_body<KQ, R, false, false, false>(E.seq, P.T, E.n, tile, lds))
  // the two h buffers stay where they are; fc1's output and the head's behind them ([maxw][R] each)
  float* act0 = lds + 2 * E.seq.Hp * R;
  float* act1 = act0 + P.maxw * R;
  const int h = E.seq.h, zs = E.zs;
  dense_rows<R>(E.w[0], E.b[0], h, h, hT, act0, false);
  dense_rows<R>(E.w[1], E.b[1], h, zs, act0, act1, false);
  if (E.rep == 0) {
    store_rows<R>(act1, E.z, zs, b0, E.n, tid);
  } else {
    for (int e = tid; e < E.rep * zs; e += blockDim.x) E.z[e] = act1[(e % zs) * R];
  }
}

// gates of the three cases from the per-modality partial projections, all [rows4 / Hp4 ..] = [T n, 4, Hp] floats; and, `fill`
// set, the constant gates cg[m] [T, 4, cHp[m]] of the zeroed encoders.  Pad units u >= h: exact zeros (P's are)
struct ZerGatesDev {
  const float* p[ZER_CASES]; float* g[ZER_CASES];
  const float* b_ih; const float* b_hh;
  int64_t total4;                              // T n 4 Hp / 4
  int h, Hp;
  float* cg[ZER_CASES]; const float* cb_ih[ZER_CASES]; const float* cb_hh[ZER_CASES];
  int ch[ZER_CASES], cHp[ZER_CASES], T, fill;
};

__global__ __launch_bounds__(256) void zeros_gates_kernel(const ZerGatesDev G) {
  const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
  const int h = G.h, Hp = G.Hp;
  const f32x4* pl = reinterpret_cast<const f32x4*>(G.p[0]);
  const f32x4* pa = reinterpret_cast<const f32x4*>(G.p[1]);
  const f32x4* pv = reinterpret_cast<const f32x4*>(G.p[2]);
  f32x4* g0 = reinterpret_cast<f32x4*>(G.g[0]);
  f32x4* g1 = reinterpret_cast<f32x4*>(G.g[1]);
  f32x4* g2 = reinterpret_cast<f32x4*>(G.g[2]);
  const int q4 = Hp >> 2;                      // 16-byte groups per gate row (Hp % 16 == 0: a group never straddles a gate)
  for (int64_t i = gtid; i < G.total4; i += gstride) {
    const int u = (int)(i % q4) * 4, g = (int)((i / q4) & 3);
    f32x4 b;
#pragma unroll
    for (int e = 0; e < 4; ++e) b[e] = (u + e < h) ? G.b_ih[g * h + u + e] + G.b_hh[g * h + u + e] : 0.0f;
    const f32x4 l = pl[i], a = pa[i], v = pv[i];
    g0[i] = (a + v) + b;
    g1[i] = (l + v) + b;
    g2[i] = (l + a) + b;
  }
  if (!G.fill) return;
#pragma unroll 1
  for (int m = 0; m < ZER_CASES; ++m) {
    const int ch = G.ch[m], cHp = G.cHp[m];
    for (int64_t i = gtid; i < (int64_t)G.T * 4 * cHp; i += gstride) {
      const int u = (int)(i % cHp), g = (int)((i / cHp) & 3);
      G.cg[m][i] = (u < ch) ? G.cb_ih[m][g * ch + u] + G.cb_hh[m][g * ch + u] : 0.0f;
    }
  }
}

__global__ __launch_bounds__(OBJ_THREADS) void zeros_finish_kernel(const ZerFinishDev P) {
  __shared__ double red[OBJ_THREADS];
  const int tid = threadIdx.x;
  double sums[ZER_ACC];
#pragma unroll
  for (int m = 0; m < ZER_CASES; ++m) {
    double v = 0.0;
    for (int i = tid; i < P.npart[m]; i += OBJ_THREADS) v += (double)P.part[m][i];
    sums[m] = finish_sum(v, red, tid);
  }
#pragma unroll
  for (int c = 0; c < ZER_CASES; ++c) {
    const double d = P.y ? label_loss_part(P.y_hat[c], P.y, P.n, P.od, P.loss_kind, tid) : 0.0;
    sums[ZER_CASES + c] = finish_sum(d, red, tid);
  }
  if (tid != 0) return;
#pragma unroll
  for (int i = 0; i < ZER_ACC; ++i) {
    if (!P.first) sums[i] += P.acc[i];
    P.acc[i] = sums[i];
  }
  if (!P.last) return;
#pragma unroll
  for (int m = 0; m < ZER_CASES; ++m) {
    P.gen[m] = (float)(sums[m] * P.inv_gen[m]);
    if (P.y) P.disc[m] = (float)(sums[ZER_CASES + m] * P.inv_disc);
  }
}

// ---------------------------------------------------------------- host
int zeros_finish_launch(const ZerFinishDev& Q, hipStream_t stream) {
  return seq_launch_kernel(zeros_finish_kernel, "zeros_finish_kernel", dim3(1), dim3(OBJ_THREADS), 0, stream, nullptr, Q);
}

static const int kZerEnc[4] = {8, 2, 20, 30};      // the canonical sizes: encoders l / a / v h = 32 / 8 / 80, ef h = 120

// the workspace, in this order (every part a multiple of 4 floats): the chunk's three partial projections and three gate sets
// and, behind the recurrences, the decoders' h in the same place; the zeroed encoders' constant gates; their factors, one row per
// chunk row; zy of the three cases; the squared-error partials; the ZER_ACC fp64 accumulators
struct ZerLayout { int64_t cgates, zc, zy, part, acc, total; };
static ZerLayout zeros_layout(int64_t T, int64_t N, const int32_t* sz, int64_t max_rows) {
  const int64_t rows = gen_rows(N, max_rows);
  const int64_t he = (int64_t)sz[0] + sz[1] + sz[2];
  ZerLayout o;
  o.cgates = std::max(rows * T * 4 * hp_of(he) * 2 * ZER_CASES, decode_ws_floats(T, N, sz[7], sz[4], sz[5], sz[6], max_rows));
  o.zc = o.cgates + T * 4 * (hp_of(sz[0]) + hp_of(sz[1]) + hp_of(sz[2]));
  o.zy = o.zc + up4(rows * sz[0]) + up4(rows * sz[1]) + up4(rows * sz[2]);
  o.part = o.zy + ZER_CASES * up4(rows * sz[3]);
  o.acc = o.part + up4(fc1_sqerr_tiles(T, rows, sz + 8));
  o.total = o.acc + up4(2 * ZER_ACC);
  return o;
}

// the launch(es) of the recurrences of one chunk: P.d[0 .. P.count) filled but for block_begin and slot
template <int R>
static int zeros_encode_launch(const char* who, ZerEncDev& P, const int* slot, int threads, size_t lds_bytes, hipStream_t stream) {
  bool canon = true;
  for (int i = 0; i < P.count; ++i) canon = canon && P.d[i].seq.hk4 == kZerEnc[slot[i]];
  if (canon) {
    int blocks = 0;
    for (int i = 0; i < P.count; ++i) {
      P.d[i].slot = slot[i]; P.d[i].block_begin = blocks;
      blocks += P.d[i].rep ? 1 : cdiv(P.d[i].n, R);
    }
    return seq_launch_kernel(zeros_encode_kernel<R, 8, 2, 20, 30>, "zeros_encode_kernel", dim3(blocks), dim3(threads), lds_bytes, stream,
                             nullptr, P);
  }
  for (int i = 0; i < P.count; ++i) {
    ZerEncDev Q = P;
    Q.d[0] = P.d[i]; Q.d[0].block_begin = 0; Q.d[0].slot = 0; Q.count = 1;
    const int rc = infer_launch_hk4(who, "zeros_encode_kernel", Q.d[0].seq,
                                    [](auto kk) { return zeros_encode_kernel<R, decltype(kk)::value, 0, 0, 0>; }, Q,
                                    Q.d[0].rep ? 1 : cdiv(Q.d[0].n, R), std::max(8 * Q.d[0].seq.Hp, 64), lds_bytes, stream);
    if (rc != MFM_OK) return rc;
  }
  return MFM_OK;
}

static int predict_zeros_klef(int T, int64_t N, const int32_t* sz, const float* params, const int64_t* offs, const float* x,
                              const void* y, float* ws, float* y_hat, float* gen, float* disc, int64_t max_rows, hipStream_t stream) {
  static const char* who = "predict zeros klef";
  MFM_REQUIRE(sz && params && offs && x && ws && y_hat && gen,
              "%s: bad arguments (sizes, params, offsets, x, workspace, y_hat and gen must not be null)", who);
  MFM_REQUIRE((y != nullptr) == (disc != nullptr), "%s: labels and disc come together (both, or both null)", who);
  int rc = infer_check_sizes(who, T, N, sz);
  if (rc != MFM_OK) return rc;
  if ((rc = infer_check_loss_kind(who, sz[12])) != MFM_OK) return rc;
  if ((rc = infer_check_aligned(who, params, x, ws)) != MFM_OK) return rc;
  if ((rc = infer_check_rows(who, N, max_rows)) != MFM_OK) return rc;
  if ((rc = infer_check_offsets(who, offs, 40, 10)) != MFM_OK) return rc;
  const int zs[ZER_CASES] = {sz[0], sz[1], sz[2]}, zys = sz[3], dm[ZER_CASES] = {sz[8], sz[9], sz[10]};
  const int od = sz[11], loss_kind = sz[12], D = dm[0] + dm[1] + dm[2], he = zs[0] + zs[1] + zs[2];
  const int hh[4] = {zs[0], zs[1], zs[2], he};
  const int rows = (int)gen_rows(N, max_rows);
  const int R = gen_tile_rows(ZER_CASES, rows);
  int maxw = std::max(he, zys), threads = 64;
  for (int i = 0; i < 4; ++i) {
    if ((rc = infer_check_resident(who, hh[i])) != MFM_OK) return rc;
    threads = std::max(threads, 8 * round_up(hh[i], 16));
  }
  size_t lds_floats = 0;
  for (int i = 0; i < 4; ++i) lds_floats = std::max(lds_floats, enc_lds_floats(hh[i], R, 2, maxw));
  const size_t lds_bytes = lds_bytes_of(lds_floats);
  if ((rc = infer_check_lds(who, lds_bytes, maxw, R)) != MFM_OK) return rc;
  const int Hpe = round_up(he, 16);
  if ((rc = infer_check_chunk(who, rows, T, std::max(D, 4 * Hpe), "projection")) != MFM_OK) return rc;
  DecLaunch Dl;
  Fc1SqLaunch S;
  if ((rc = decode_factors_prepare(who, T, N, sz, params, offs + 40, ws, max_rows, Dl)) != MFM_OK) return rc;
  if ((rc = fc1_sqerr_prepare(who, Dl, N, S)) != MFM_OK) return rc;
  const int* col = S.col;                     // the first column of each modality in x

  const ZerLayout lay = zeros_layout(T, N, sz, max_rows);
  const int64_t gsz = (int64_t)rows * T * 4 * Hpe;        // one partial projection / one gate set of a full chunk
  float* zc[ZER_CASES]; float* zyb[ZER_CASES];
  {
    float* p = ws + lay.zc;
    for (int m = 0; m < ZER_CASES; ++m) { zc[m] = p; p += up4((int64_t)rows * zs[m]); }
    p = ws + lay.zy;
    for (int c = 0; c < ZER_CASES; ++c) { zyb[c] = p; p += up4((int64_t)rows * zys); }
  }
  float* part = ws + lay.part;
  double* acc = reinterpret_cast<double*>(ws + lay.acc);      // (a multiple of 4 floats from a 16-byte aligned base)

  // the ef encoder (the fourth of the 40 encoder offsets' groups), once per case; then the zeroed encoders
  ZerEncDev PE;
  memset(&PE, 0, sizeof(PE));
  ZerGatesDev G;
  memset(&G, 0, sizeof(G));
  int slot[ZER_LSTMS];
  {
    const int64_t* o = offs + 30;
    for (int c = 0; c < ZER_CASES; ++c) {
      ZerOne& E = PE.d[c];
      seq_fill(E.seq, params + o[0], params + o[1], params + o[2], params + o[3], he, 0);
      G.p[c] = ws + c * gsz;
      G.g[c] = E.seq.gates = ws + (ZER_CASES + c) * gsz;
      E.w[0] = params + o[4]; E.b[0] = params + o[5]; E.w[1] = params + o[6]; E.b[1] = params + o[7];
      E.zs = zys; E.z = zyb[c]; E.rep = 0;
      slot[c] = 3;
    }
    G.b_ih = params + o[2]; G.b_hh = params + o[3]; G.h = he; G.Hp = Hpe; G.T = T;
    float* cg = ws + lay.cgates;
    for (int m = 0; m < ZER_CASES; ++m) {
      ZerOne& E = PE.d[ZER_CASES + m];
      const int64_t* om = offs + 10 * m;
      seq_fill(E.seq, params + om[0], params + om[1], params + om[2], params + om[3], zs[m], 0);
      E.seq.gates = cg;
      G.cg[m] = cg; G.cb_ih[m] = params + om[2]; G.cb_hh[m] = params + om[3]; G.ch[m] = zs[m]; G.cHp[m] = E.seq.Hp;
      cg += (int64_t)T * 4 * E.seq.Hp;
      E.w[0] = params + om[4]; E.b[0] = params + om[5]; E.w[1] = params + om[6]; E.b[1] = params + om[7];
      E.zs = zs[m]; E.z = zc[m]; E.n = 1; E.rep = rows;
      slot[ZER_CASES + m] = m;
    }
  }
  PE.T = T; PE.maxw = maxw;
  const SeqDev& ef = PE.d[0].seq;

  ZerFinishDev Q;
  memset(&Q, 0, sizeof(Q));
  for (int m = 0; m < ZER_CASES; ++m) Q.inv_gen[m] = S.inv_gen[m];
  Q.acc = acc; Q.gen = gen; Q.disc = disc;
  Q.inv_disc = inv_label_count(loss_kind, N, od);
  Q.od = od; Q.loss_kind = loss_kind;

  for (int64_t n0 = 0; n0 < N; n0 += rows) {
    const int n = (int)std::min<int64_t>(rows, N - n0);
    const bool whole = n == N, first = n0 == 0;
    // P_m[t][i][g][u] = x_m[t][n0 + i] . W_ih[g h + u][columns of m]; pad units u >= h exact zeros
    rc = gemm_group_each(ZER_CASES * (whole ? 1 : T), stream, [&](int p, MfmGemmDesc& d) {
      const int m = p % ZER_CASES, t = p / ZER_CASES;
      d.a = x + ((int64_t)t * N + n0) * D + col[m]; d.a_sm = D; d.a_sk = 1;
      d.b = ef.w_ih + col[m]; d.b_sz = (int64_t)he * D; d.b_sn = D; d.b_sk = 1;
      d.c = const_cast<float*>(G.p[m]) + (int64_t)t * n * 4 * Hpe; d.c_sz = Hpe; d.ldc = 4 * (int64_t)Hpe;
      d.m = whole ? T * n : n; d.n = Hpe; d.n_valid = he; d.k = dm[m]; d.batch = 4; d.split_k = 1;
      d.alpha = 1.0f;
    });
    if (rc != MFM_OK) return rc;
    G.total4 = (int64_t)T * n * Hpe;         // (T n 4 Hp floats, four at a time)
    G.fill = first;
    const int gblocks = (int)std::min<int64_t>((G.total4 + 255) / 256, 8 * (int64_t)device_cus());
    zeros_gates_kernel<<<dim3(gblocks), dim3(256), 0, stream>>>(G);
    MFM_LAUNCH_CHECK("zeros_gates_kernel");
    for (int c = 0; c < ZER_CASES; ++c) PE.d[c].n = n;
    PE.count = first ? ZER_LSTMS : ZER_CASES;      // the zeroed encoders' rows do not depend on the chunk: the first one computes them
    rc = (R == 1) ? zeros_encode_launch<1>(who, PE, slot, threads, lds_bytes, stream)
                  : zeros_encode_launch<4>(who, PE, slot, threads, lds_bytes, stream);
    if (rc != MFM_OK) return rc;
    // (the projections and gates are dead behind the recurrences: the decoders' h takes their place)
    DecodeDev& PD = Dl.P;
    PD.n = n;
    for (int c = 0; c < ZER_CASES; ++c) {
      PD.d[c].zm = zc[c]; PD.d[c].zy = zyb[c];
      PD.d[c].y_hat = y_hat + ((int64_t)c * N + n0) * od;
    }
    if ((rc = decode_factors_launch(who, PD, Dl.R, Dl.threads, Dl.lds_bytes, stream)) != MFM_OK) return rc;
    if ((rc = fc1_sqerr_chunk(S, x, n0, n, part, Q.part, Q.npart, stream)) != MFM_OK) return rc;
    for (int c = 0; c < ZER_CASES; ++c) Q.y_hat[c] = PD.d[c].y_hat;
    Q.y = labels_at(y, loss_kind, n0, od);
    Q.n = n; Q.first = first; Q.last = n0 + n == N;
    if ((rc = zeros_finish_launch(Q, stream)) != MFM_OK) return rc;
  }
  return MFM_OK;
}

}  // namespace mfm

extern "C" int64_t mfm_predict_zeros_klef_workspace_floats(int32_t T, int64_t N, const int32_t* sizes, int64_t max_rows) {
  if (T < 1 || N < 1 || !sizes || max_rows < 0) return 0;
  for (int i = 0; i < 12; ++i)
    if (sizes[i] < 1) return 0;
  return mfm::zeros_layout(T, N, sizes, max_rows).total;
}

extern "C" int mfm_predict_zeros_klef(int32_t T, int64_t N, const int32_t* sizes, const float* params, const int64_t* offsets,
                                      const float* x, const void* y, float* workspace, float* y_hat, float* gen, float* disc,
                                      int64_t max_rows, void* stream) {
  return mfm::predict_zeros_klef(T, N, sizes, params, offsets, x, y, workspace, y_hat, gen, disc, max_rows, (hipStream_t)stream);
}
