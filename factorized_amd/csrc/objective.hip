// The full validation objective of MFM_KL_EF (include/mfm_hip.h, mfm_objective_klef): what every driver of the reference reports
// for a validation split (mfm_mosi.py:319-324, :724-726, :826-845),
//     loss = disc + lda_xl mse_l + lda_xa mse_a + lda_xv mse_v + lda_mmd reg
// with its five terms, from the deterministic eval forward (mfm_model.py:619-660) -- no plan, no training workspace, and no x_hat:
// the reconstructions exist in registers only.  Per row chunk, five launches on one stream:
//   1. + 2. the encoder half exactly as mfm_encode_klef launches it (generate.hip: the projection GEMM, encode_klef_kernel); the
//      chunk's means and log-variances go to the workspace;
//   3. the decoder recurrences exactly as mfm_decode_factors launches them (decode_factors_kernel on the means: h_t of the
//      three decoders and y_hat into the workspace);
//   4. fc1_sqerr_kernel: workgroup (decoder m, 64-row tile of the T n rows, 64-column tile of d_m) stages its rows of h and
//      its rows of W_fc1 in LDS, forms x_hat = h W^T + b on v_mfma_f32_16x16x4_f32 (4 waves x 16 rows x up to 4 column
//      fragments), subtracts the matching slice of x straight from HBM (modality m's columns of the chunk's rows inside
//      [T, N, D]: scalar loads, no alignment assumed), squares, and adds up: lane -> wave (DPP) -> workgroup (LDS, fixed order).
//      One fp32 partial per workgroup into its own slot.  Rows and columns past the edge are staged as zeros AND masked in the
//      epilogue: they contribute exactly 0;
//   5. objective_finish_kernel, one workgroup: the chunk's squared-error partials per modality, its KLD sum
//      (1 + logvar - mu^2 - exp(logvar), mfm_model.loss_KLD) and its label-loss sum (|y_hat - y|, or logsumexp - picked as in
//      predict.hip), each in a fixed order (thread-strided, then one LDS tree) in fp64, into five fp64 accumulators of the
//      workspace -- the first chunk stores, the others add, in stream order.  Behind the last chunk it divides by the counts of
//      the WHOLE split, forms the total and writes the six floats.
// The chunks' working set does not grow with N beyond the row cap.  No float atomics: the result is bit-identical from run to
// run for a given (T, N, max_rows).
#include "infer_dev.h"

namespace mfm {

static_assert(OBJ_BM == OBJ_BN && OBJ_BM * 4 == OBJ_THREADS, "one staging loop fills both LDS tiles; a wave owns 16 rows");

__global__ __launch_bounds__(OBJ_THREADS) void fc1_sqerr_kernel(const Fc1SqDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float red[OBJ_THREADS / 64];
  const int tid = threadIdx.x, bid = blockIdx.x;
  const int m = (bid >= P.it[2].tile_begin) ? 2 : ((bid >= P.it[1].tile_begin) ? 1 : 0);
  const Fc1SqItem& I = P.it[m];
  const int tile = bid - I.tile_begin;
  const int rt = tile / I.col_tiles, ct = tile - rt * I.col_tiles;
  const int r0 = rt * OBJ_BM, c0 = ct * OBJ_BN;
  const int h = I.h, d = I.d, K4 = (h + 3) & ~3;
  // row stride K4 + 2 floats: half of it is odd, so the 16 rows x 2 k of a 32-lane read group fall on 32 different banks
  const int ld = K4 + 2;
  float* Hs = lds;
  float* Ws = lds + OBJ_BM * ld;
  for (int e = tid; e < OBJ_BM * K4; e += OBJ_THREADS) {
    const int r = e / K4, k = e - r * K4;
    const bool in_k = k < h;
    Hs[r * ld + k] = (in_k && r0 + r < P.M) ? I.hs[(int64_t)(r0 + r) * I.Hp + k] : 0.0f;
    Ws[r * ld + k] = (in_k && c0 + r < d) ? I.w[(int64_t)(c0 + r) * h + k] : 0.0f;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63, lr = lane & 15, kq = lane >> 4;
  const int nfrag = min(OBJ_BN / 16, (d - c0 + 15) / 16);
  f32x4 acc[OBJ_BN / 16];
#pragma unroll
  for (int f = 0; f < OBJ_BN / 16; ++f) acc[f] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  const float* ap = Hs + (wave * 16 + lr) * ld + kq;
  const float* bp = Ws + lr * ld + kq;
  for (int k0 = 0; k0 < K4; k0 += 4) {
    const float a = ap[k0];
#pragma unroll
    for (int f = 0; f < OBJ_BN / 16; ++f)
      if (f < nfrag) acc[f] = mma16x16x4(a, bp[f * 16 * ld + k0], acc[f]);
  }
  // result register i of lane (lr, kq): row wave * 16 + kq * 4 + i, column f * 16 + lr
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = r0 + wave * 16 + kq * 4 + i;
    if (row < P.M) {
      const int t = row / P.n, ri = row - t * P.n;
      const float* xr = I.x + ((int64_t)t * P.N + ri) * P.D;
#pragma unroll
      for (int f = 0; f < OBJ_BN / 16; ++f) {
        const int col = c0 + f * 16 + lr;
        if (f < nfrag && col < d) {
          const float v = (acc[f][i] + I.bias[col]) - xr[col];
          s = fmaf(v, v, s);
        }
      }
    }
  }
  s = wave_sum_dpp(s);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (tid == 0) I.partials[tile] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(OBJ_THREADS) void objective_finish_kernel(const ObjFinishDev P) {
  __shared__ double red[OBJ_THREADS];
  const int tid = threadIdx.x;
  double sums[OBJ_ACC];
#pragma unroll
  for (int m = 0; m < INFER_DEC; ++m) {
    double v = 0.0;
    for (int i = tid; i < P.npart[m]; i += OBJ_THREADS) v += (double)P.part[m][i];
    sums[m] = finish_sum(v, red, tid);
  }
  double kld = 0.0;
#pragma unroll
  for (int e = 0; e < INFER_ENC; ++e)
    for (int i = tid; i < P.nz[e]; i += OBJ_THREADS) {
      const float mu = P.mu[e][i], lv = P.lv[e][i];
      kld += (double)(1.0f + lv - mu * mu - expf(lv));
    }
  sums[3] = finish_sum(kld, red, tid);
  const double disc = label_loss_part(P.y_hat, P.y, P.n, P.od, P.loss_kind, tid);
  sums[4] = finish_sum(disc, red, tid);
  if (tid != 0) return;
#pragma unroll
  for (int i = 0; i < OBJ_ACC; ++i) {
    if (!P.first) sums[i] += P.acc[i];
    P.acc[i] = sums[i];
  }
  if (!P.last) return;
  const float d = (float)(sums[4] * P.inv_disc);
  const float gl = (float)(sums[0] * P.inv_gen[0]), ga = (float)(sums[1] * P.inv_gen[1]), gv = (float)(sums[2] * P.inv_gen[2]);
  const float reg = (float)(-0.5 * sums[3]);
  P.out[0] = d + P.lda[0] * gl + P.lda[1] * ga + P.lda[2] * gv + P.lda[3] * reg;
  P.out[1] = d; P.out[2] = gl; P.out[3] = ga; P.out[4] = gv; P.out[5] = reg;
}

// ---------------------------------------------------------------- host
int objective_finish_launch(const ObjFinishDev& Q, hipStream_t stream) {
  return seq_launch_kernel(objective_finish_kernel, "objective_finish_kernel", dim3(1), dim3(OBJ_THREADS), 0, stream, nullptr, Q);
}

int fc1_sqerr_prepare(const char* who, const DecLaunch& L, int64_t N, Fc1SqLaunch& S) {
  const int T = L.P.T;
  MFM_REQUIRE(fc1_sqerr_tiles(T, L.rows, L.dm) < ((int64_t)1 << 31), "%s: a chunk of %d rows x %d steps is too large; pass a row cap", who, L.rows, T);
  memset(&S, 0, sizeof(S));
  S.hmax = 1;
  for (int m = 0; m < INFER_DEC; ++m) {
    const SeqDev& s = L.P.d[m].seq;
    Fc1SqItem& I = S.F.it[m];
    I.hs = s.hs; I.w = L.fcw[m]; I.bias = L.fcb[m];
    I.d = L.dm[m]; I.h = s.h; I.Hp = s.Hp; I.col_tiles = cdiv(L.dm[m], OBJ_BN);
    S.hmax = std::max(S.hmax, s.h);
    S.col[m] = S.F.D;
    S.F.D += L.dm[m];
    S.inv_gen[m] = 1.0 / ((double)T * (double)N * (double)L.dm[m]);
  }
  S.F.N = N; S.T = T;
  return MFM_OK;
}

int fc1_sqerr_chunk(Fc1SqLaunch& S, const float* x, int64_t n0, int n, float* partials, const float** part, int* npart, hipStream_t stream) {
  Fc1SqDev& F = S.F;
  F.M = S.T * n; F.n = n;
  const int row_tiles = cdiv(F.M, OBJ_BM);
  int tiles = 0;
  for (int m = 0; m < INFER_DEC; ++m) {
    Fc1SqItem& I = F.it[m];
    I.x = x + n0 * F.D + S.col[m];
    I.tile_begin = tiles; I.partials = partials + tiles;
    part[m] = I.partials; npart[m] = row_tiles * I.col_tiles;
    tiles += npart[m];
  }
  const size_t lds_bytes = (size_t)(OBJ_BM + OBJ_BN) * (round_up(S.hmax, 4) + 2) * sizeof(float);
  return seq_launch_kernel(fc1_sqerr_kernel, "fc1_sqerr_kernel", dim3(tiles), dim3(OBJ_THREADS), lds_bytes, stream, nullptr, F);
}

// the workspace, in this order (every part a multiple of 4 floats): the chunk's x-projections and, behind the encoders, the
// decoders' h in the same place; its eight factors; its y_hat; its squared-error partials; the OBJ_ACC fp64 accumulators
struct ObjLayout { int64_t seq, z, y_hat, part, total; };
static ObjLayout objective_layout(int64_t T, int64_t N, const int32_t* sz, int64_t max_rows) {
  const int64_t rows = gen_rows(N, max_rows);
  ObjLayout o;
  o.seq = std::max(encode_ws_floats(T, N, sz[0], sz[1], sz[2], max_rows), decode_ws_floats(T, N, sz[7], sz[4], sz[5], sz[6], max_rows));
  o.z = o.seq;
  o.y_hat = o.z + 2 * (up4(rows * sz[0]) + up4(rows * sz[1]) + up4(rows * sz[2]) + up4(rows * sz[3]));
  o.part = o.y_hat + up4(rows * sz[11]);
  o.total = o.part + up4(fc1_sqerr_tiles(T, rows, sz + 8)) + up4(2 * OBJ_ACC);
  return o;
}

static int objective_klef(int T, int64_t N, const int32_t* sz, const float* lambdas, const float* params, const int64_t* offs,
                          const float* x, const void* y, float* ws, float* out, int64_t max_rows, hipStream_t stream) {
  static const char* who = "objective klef";
  MFM_REQUIRE(sz && lambdas && params && offs && x && y && ws && out,
              "%s: bad arguments (sizes, lambdas, params, offsets, x, y, workspace and out must not be null)", who);
  int rc = infer_check_sizes(who, T, N, sz);
  if (rc != MFM_OK) return rc;
  if ((rc = infer_check_loss_kind(who, sz[12])) != MFM_OK) return rc;
  if ((rc = infer_check_aligned(who, params, x, ws)) != MFM_OK) return rc;
  const int zs[INFER_ENC] = {sz[0], sz[1], sz[2], sz[3]};
  const int od = sz[11], loss_kind = sz[12];
  EncLaunch E;
  DecLaunch Dl;
  Fc1SqLaunch S;
  if ((rc = encode_klef_prepare(who, T, N, sz[8], sz[9], sz[10], zs[0], zs[1], zs[2], zs[3], params, offs, ws, max_rows, E)) != MFM_OK) return rc;
  if ((rc = decode_factors_prepare(who, T, N, sz, params, offs + 40, ws, max_rows, Dl)) != MFM_OK) return rc;
  if ((rc = fc1_sqerr_prepare(who, Dl, N, S)) != MFM_OK) return rc;
  const int rows = E.rows;

  const ObjLayout lay = objective_layout(T, N, sz, max_rows);
  float* zbuf[2 * INFER_ENC];
  {
    float* p = ws + lay.z;
    for (int half = 0; half < 2; ++half)
      for (int i = 0; i < INFER_ENC; ++i) { zbuf[4 * half + i] = p; p += up4((int64_t)rows * zs[i]); }
  }
  float* y_hat = ws + lay.y_hat;
  float* part = ws + lay.part;
  double* acc = reinterpret_cast<double*>(ws + lay.total - up4(2 * OBJ_ACC));      // (a multiple of 4 floats from a 16-byte aligned base)

  ObjFinishDev Q;
  memset(&Q, 0, sizeof(Q));
  for (int m = 0; m < INFER_DEC; ++m) Q.inv_gen[m] = S.inv_gen[m];
  for (int i = 0; i < INFER_ENC; ++i) { Q.mu[i] = zbuf[i]; Q.lv[i] = zbuf[4 + i]; }
  Q.y_hat = y_hat; Q.acc = acc; Q.out = out;
  Q.inv_disc = inv_label_count(loss_kind, N, od);
  for (int i = 0; i < 4; ++i) Q.lda[i] = lambdas[i];
  Q.od = od; Q.loss_kind = loss_kind;

  for (int64_t n0 = 0; n0 < N; n0 += rows) {
    const int n = (int)std::min<int64_t>(rows, N - n0);
    if ((rc = encode_klef_chunk(E, x, N, n0, n, zbuf, stream)) != MFM_OK) return rc;
    // (the x-projections are dead behind the encoders' launch: the decoders' h takes their place)
    if ((rc = decode_factors_chunk(who, Dl, zbuf, y_hat, n, stream)) != MFM_OK) return rc;
    if ((rc = fc1_sqerr_chunk(S, x, n0, n, part, Q.part, Q.npart, stream)) != MFM_OK) return rc;
    for (int i = 0; i < INFER_ENC; ++i) Q.nz[i] = n * zs[i];
    Q.y = labels_at(y, loss_kind, n0, od);
    Q.n = n; Q.first = n0 == 0; Q.last = n0 + n == N;
    if ((rc = objective_finish_launch(Q, stream)) != MFM_OK) return rc;
  }
  return MFM_OK;
}

}  // namespace mfm

extern "C" int64_t mfm_objective_klef_workspace_floats(int32_t T, int64_t N, const int32_t* sizes, int64_t max_rows) {
  if (T < 1 || N < 1 || !sizes || max_rows < 0) return 0;
  for (int i = 0; i < 12; ++i)
    if (sizes[i] < 1) return 0;
  return mfm::objective_layout(T, N, sizes, max_rows).total;
}

extern "C" int mfm_objective_klef(int32_t T, int64_t N, const int32_t* sizes, const float* lambdas, const float* params,
                                  const int64_t* offsets, const float* x, const void* y, float* workspace, float* out,
                                  int64_t max_rows, void* stream) {
  return mfm::objective_klef(T, N, sizes, lambdas, params, offsets, x, y, workspace, out, max_rows, (hipStream_t)stream);
}
