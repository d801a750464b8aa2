// Prediction-only path of MFM_KL_EF (include/mfm_hip.h, mfm_predict_klef): what y_hat depends on and nothing else.
//
// In eval mode MFM_KL_EF.forward (mfm_model.py:637-657) computes y_hat from ONE of its seven recurrences:
//     ef_last = ef_encoder(x)  ->  zy = last_to_zy_fc1(ef_last)  (the mean; forward() does not sample)
//     fy = relu(zy_to_fy_fc2(relu(zy_to_fy_fc1(zy))))            (dropout is the identity)
//     y_hat = fy_to_y_fc2(relu(fy_to_y_fc1(fy)))
// The three modality encoders, the logvar heads, the KL term, the modalities' z -> f MLPs, the decoders and their fc1 are dead
// work for evaluate() / predict(), and so is every record a backward would read.  Two launches per row chunk:
//   1. the input projection X[T n, D] W_ih^T + b_ih + b_hh -> gates [T, n, 4, Hp] (the grouped fp32 GEMM, gemm.hip), into the
//      caller's workspace;
//   2. predict_klef_kernel: a workgroup owns R batch rows (R chosen as seq_small_launch chooses it), runs the T-step
//      recurrence with small_fwd_body<.., REC = false> -- h / c stay on chip, no hs / cs / gate record leaves for HBM -- and
//      then, on the tile's last hidden states still in LDS, the encoder's fc1, the zy head, the fy MLP and the classifier
//      (dense_rows, dense_rows_dev.h: a quad of lanes per output column, the weights straight from L2, activations in LDS).  It writes
//      y_hat and, with labels, its rows' part of the discriminative loss.
// Loss: one partial per workgroup (plain sums in a fixed order), stored to the workspace; behind it lane 0 draws an arrival
// ticket (agent-scope fetch_add, acquire-release -- the pattern of keep_best.hip).  The workgroup that draws the LAST ticket
// of the call (the chunks' launches share one ticket word and one partial array) adds all partials in a fixed order --
// lane l of its first wave takes partials l, l + 64, ... in ascending order, then one fixed DPP / readlane tree -- writes the
// mean to the caller's device float and puts the ticket back to 0.  No float atomics touch the result: the value is
// bit-identical from run to run.  Nobody waits or spins.
// Any N >= 1, T >= 1: the grid is ceil(n / R) per chunk; rows beyond the chunk are neither read (clamped re-reads of the last
// row inside the body) nor written.
#include <algorithm>

#include "lstm_seq_small_dev.h"
#include "dense_rows_dev.h"

namespace mfm {

#define PRED_LAYERS 6          // ef_encoder.fc1, last_to_zy_fc1, zy_to_fy_fc1, zy_to_fy_fc2, fy_to_y_fc1, fy_to_y_fc2

struct PredictDev {
  SeqDev seq;                                  // gates (the x-projections, read only), w_hh, h, Hp, hk4
  const float* w[PRED_LAYERS]; const float* b[PRED_LAYERS];
  int K[PRED_LAYERS], N[PRED_LAYERS], relu[PRED_LAYERS];
  const void* y; float* y_hat;                 // this chunk's labels (null: none) and outputs [n, od]
  float* partials; int* ticket; float* loss;   // workspace: one partial per workgroup of the call, the ticket word; the result
  int T, n, od, loss_kind, maxw;               // n: rows of this chunk
  int wg_base, wg_total;                       // this launch's first slot in `partials`, workgroups of the whole call
  float inv;                                   // 1 / (N od) (L1) or 1 / N (CE) over the WHOLE call
};

template <int KQ, int R>
__global__ __launch_bounds__(1024) void predict_klef_kernel(const PredictDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int HKB = (4 * KQ + 15) / 16 * 16;
  const int tid = threadIdx.x;
  const int tile = blockIdx.x, b0 = tile * R;
  const float* hT = small_fwd_body<KQ, R, false, false, false>(P.seq, P.T, P.n, tile, lds);
  // the two h buffers stay where they are; the activations of the heads ping-pong behind them ([maxw][R] each)
  float* act0 = lds + 2 * HKB * R;
  float* act1 = act0 + P.maxw * R;
  const float* in = hT;
#pragma unroll 1
  for (int l = 0; l < PRED_LAYERS; ++l) {
    float* out = (l & 1) ? act1 : act0;
    dense_rows<R>(P.w[l], P.b[l], P.K[l], P.N[l], in, out, P.relu[l] != 0);
    in = out;
  }
  // in == act1: y_hat of the tile as [od][R]
  const int od = P.od;
  for (int e = tid; e < od * R; e += blockDim.x) {
    const int r = e / od, o = e - r * od;
    if (b0 + r < P.n) P.y_hat[(int64_t)(b0 + r) * od + o] = in[o * R + r];
  }
  if (!P.y || !P.loss || tid >= 64) return;       // (the first wave alone goes on)
  float part = 0.0f;
  if (P.loss_kind == 0) {
    const float* yt = reinterpret_cast<const float*>(P.y);
    for (int e = tid; e < od * R; e += 64) {
      const int r = e / od, o = e - r * od;
      if (b0 + r < P.n) part += fabsf(in[o * R + r] - yt[(int64_t)(b0 + r) * od + o]);
    }
  } else if (tid < R && b0 + tid < P.n) {
    const int64_t lab = reinterpret_cast<const int64_t*>(P.y)[b0 + tid];
    float mx = in[tid];
    for (int o = 1; o < od; ++o) mx = fmaxf(mx, in[o * R + tid]);
    float se = 0.0f;
    for (int o = 0; o < od; ++o) se += expf(in[o * R + tid] - mx);
    const int lc = (int)min(max(lab, (int64_t)0), (int64_t)(od - 1));      // (a label outside [0, od) must not index outside LDS)
    part = (logf(se) + mx) - in[lc * R + tid];
  }
  part = wave_sum_dpp(part);
  int drawn = 0;
  if (tid == 0) {
    __hip_atomic_store(P.partials + P.wg_base + tile, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    drawn = __hip_atomic_fetch_add(P.ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  }
  drawn = __builtin_amdgcn_readfirstlane(drawn);
  if (drawn != P.wg_total - 1) return;
  // the last arriver of the call: every partial was stored in front of its workgroup's draw
  float s = 0.0f;
  for (int i = tid; i < P.wg_total; i += 64) s += __hip_atomic_load(P.partials + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  s = wave_sum_dpp(s);
  if (tid == 0) {
    __hip_atomic_store(P.loss, s * P.inv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(P.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

static int64_t predict_rows(int64_t N, int64_t max_rows) { return (max_rows > 0 && max_rows < N) ? max_rows : N; }

// floats: the x-projections of one row chunk, one loss partial per row (a one-row tile each at most), the ticket word (+ pad)
static int64_t predict_ws_floats(int64_t T, int64_t N, int64_t h, int64_t max_rows) {
  const int64_t Hp = (h + 15) / 16 * 16;
  return predict_rows(N, max_rows) * T * 4 * Hp + N + 4;
}

static size_t predict_lds_bytes(int h, int R, int maxw) {
  const size_t HKB = (size_t)round_up(4 * round_up(cdiv(h, 4), 2), 16);
  const size_t hh = (R == 1 && (h & 3) == 0) ? 0 : (size_t)h * h;       // the weight staging panel of small_fwd_body
  const size_t rec = (2 * 6 + 2 * 4) * HKB * R;                          // its record / x-projection buffers (layout kept)
  const size_t heads = 2 * (size_t)maxw * R;
  const size_t need = 2 * HKB * R + std::max(std::max(2 * hh, rec), heads);
  return (need * sizeof(float) + 15) / 16 * 16;
}

template <int R>
static int predict_launch_r(const PredictDev& P, int grid, int threads, size_t lds_bytes, hipStream_t stream) {
#define PRED_CASE(KK, ...) \
  case KK: return seq_launch_kernel(predict_klef_kernel<KK, R>, "predict_klef_kernel", dim3(grid), dim3(threads), lds_bytes, stream, nullptr, P);
  switch (P.seq.hk4) { MFM_HK4_CASES(PRED_CASE) }
#undef PRED_CASE
  set_error("predict klef: no kernel for h = %d", P.seq.h);
  return MFM_ERR_UNSUPPORTED;
}

static int predict_klef(int T, int64_t N, int D, int h, int zy, int fy, int od, int loss_kind, const float* params,
                        const int64_t* offs, const float* x, const void* y, float* ws, float* y_hat, float* loss_dev,
                        int64_t max_rows, hipStream_t stream) {
  static const char* who = "predict klef";
  MFM_REQUIRE(T >= 1 && N >= 1 && D >= 1 && h >= 1 && zy >= 1 && fy >= 1 && od >= 1, "%s: sizes must be positive (T %d, N %lld, D %d, h %d, zy %d, fy %d, output_dim %d)",
              who, T, (long long)N, D, h, zy, fy, od);
  MFM_REQUIRE(loss_kind == 0 || loss_kind == 1, "%s: unknown loss kind %d (0 = L1, 1 = cross entropy)", who, loss_kind);
  MFM_REQUIRE(params && offs && x && ws && y_hat, "%s: bad arguments (params, offsets, x, workspace and y_hat must not be null)", who);
  MFM_REQUIRE((((uintptr_t)params | (uintptr_t)x | (uintptr_t)ws) & 15) == 0, "%s: params, x and workspace must be 16-byte aligned", who);
  MFM_REQUIRE(max_rows >= 0, "%s: row cap %lld (0 = the whole split in one chunk)", who, (long long)max_rows);
  MFM_REQUIRE(N < ((int64_t)1 << 24), "%s: N = %lld rows (at most 2^24 - 1)", who, (long long)N);
  for (int i = 0; i < 4 + 2 * PRED_LAYERS; ++i)
    MFM_REQUIRE(offs[i] >= 0 && (i >= 2 || (offs[i] & 3) == 0), "%s: parameter offset %d is %lld (not negative; the LSTM weights 16-byte aligned)", who, i, (long long)offs[i]);
  const int maxw = std::max(std::max(h, zy), std::max(fy, od));
  const int rows = (int)predict_rows(N, max_rows);
  const int R = ((long)rows < 6L * device_cus()) ? 1 : 4;
  // what the on-chip recurrence does not cover is refused: the caller runs the training forward instead
  if (h > MFM_SEQ_MAX_RESIDENT_H) {
    set_error("%s: hidden size h = %d is beyond the register-resident recurrence (at most %d)", who, h, MFM_SEQ_MAX_RESIDENT_H);
    return MFM_ERR_UNSUPPORTED;
  }
  const size_t lds_bytes = predict_lds_bytes(h, R, maxw);
  if (lds_bytes > 160 * 1024) {
    set_error("%s: %zu bytes of LDS per workgroup (h = %d, widest layer %d, %d rows per workgroup) exceed the 160 KB of a CU", who, lds_bytes, h, maxw, R);
    return MFM_ERR_UNSUPPORTED;
  }
  MFM_REQUIRE((int64_t)rows * T * D < ((int64_t)1 << 31) && (int64_t)rows * T * 4 * round_up(h, 16) < ((int64_t)1 << 31),
              "%s: a chunk of %d rows x %d steps is too large for one projection; pass a row cap", who, rows, T);

  const int Hp = round_up(h, 16);
  float* gates = ws;
  float* partials = ws + (int64_t)rows * T * 4 * Hp;
  int* ticket = reinterpret_cast<int*>(partials + N);
  const bool with_loss = y && loss_dev;
  int wg_total = 0;
  for (int64_t n0 = 0; n0 < N; n0 += rows) wg_total += cdiv((int)std::min<int64_t>(rows, N - n0), R);
  // (a call that ended in an error between two chunks may have left arrivals behind)
  if (with_loss) MFM_HIP_CHECK(hipMemsetAsync(ticket, 0, sizeof(int), stream));

  PredictDev P;
  memset(&P, 0, sizeof(P));
  P.seq.gates = gates; P.seq.w_hh = params + offs[1]; P.seq.w_ih = params + offs[0];
  P.seq.b_ih = params + offs[2]; P.seq.b_hh = params + offs[3];
  P.seq.h = h; P.seq.Hp = Hp; P.seq.hk4 = round_up(cdiv(h, 4), 2); P.seq.is_dec = 0;
  const int K[PRED_LAYERS] = {h, h, zy, fy, fy, fy}, Nn[PRED_LAYERS] = {h, zy, fy, fy, fy, od};
  const int relu[PRED_LAYERS] = {0, 0, 1, 1, 1, 0};
  for (int l = 0; l < PRED_LAYERS; ++l) {
    P.w[l] = params + offs[4 + 2 * l]; P.b[l] = params + offs[5 + 2 * l];
    P.K[l] = K[l]; P.N[l] = Nn[l]; P.relu[l] = relu[l];
  }
  P.T = T; P.od = od; P.loss_kind = loss_kind; P.maxw = maxw;
  P.partials = partials; P.ticket = ticket; P.loss = with_loss ? loss_dev : nullptr;
  P.wg_total = wg_total;
  P.inv = loss_kind == 0 ? (float)(1.0 / ((double)N * (double)od)) : (float)(1.0 / (double)N);
  const int threads = std::max(8 * Hp, 64);

  int wg_base = 0;
  for (int64_t n0 = 0; n0 < N; n0 += rows) {
    const int n = (int)std::min<int64_t>(rows, N - n0);
    // gates[t][i][g][u] = x[t][n0 + i] . W_ih[g h + u] + b_ih + b_hh; pad units u >= h exact zeros
    MfmGemmDesc g[MFM_GEMM_MAXP];
    const bool whole = n == N;           // one chunk: the T * N rows of x are one matrix
    const int nprob = whole ? 1 : T;
    for (int t0 = 0; t0 < nprob; t0 += MFM_GEMM_MAXP) {
      const int cnt = std::min(MFM_GEMM_MAXP, nprob - t0);
      memset(g, 0, sizeof(MfmGemmDesc) * cnt);
      for (int i = 0; i < cnt; ++i) {
        const int t = t0 + i;
        MfmGemmDesc& d = g[i];
        d.a = x + ((int64_t)t * N + n0) * D; d.a_sm = D; d.a_sk = 1; d.a_sz = 0;
        d.b = P.seq.w_ih; d.b_sz = (int64_t)h * D; d.b_sn = D; d.b_sk = 1;
        d.c = gates + (int64_t)t * n * 4 * Hp; d.c_sz = Hp; d.ldc = 4 * (int64_t)Hp;
        d.bias = P.seq.b_ih; d.bias2 = P.seq.b_hh; d.bias_sz = h;
        d.m = whole ? T * n : n; d.n = Hp; d.n_valid = h; d.k = D; d.batch = 4; d.split_k = 1;
        d.alpha = 1.0f;
      }
      const int rc = gemm_group_launch(g, cnt, stream);
      if (rc != MFM_OK) return rc;
    }
    P.n = n;
    P.y = !with_loss ? nullptr
                     : (loss_kind == 0 ? (const void*)(reinterpret_cast<const float*>(y) + n0 * od)
                                       : (const void*)(reinterpret_cast<const int64_t*>(y) + n0));
    P.y_hat = y_hat + n0 * od;
    P.wg_base = wg_base;
    const int grid = cdiv(n, R);
    const int rc = (R == 1) ? predict_launch_r<1>(P, grid, threads, lds_bytes, stream)
                            : predict_launch_r<4>(P, grid, threads, lds_bytes, stream);
    if (rc != MFM_OK) return rc;
    wg_base += grid;
  }
  return MFM_OK;
}

}  // namespace mfm

extern "C" int64_t mfm_predict_klef_workspace_floats(int32_t T, int64_t N, int32_t h, int64_t max_rows) {
  if (T < 1 || N < 1 || h < 1 || max_rows < 0) return 0;
  return mfm::predict_ws_floats(T, N, h, max_rows);
}

extern "C" int mfm_predict_klef(int32_t T, int64_t N, int32_t D, int32_t h, int32_t zy, int32_t fy, int32_t output_dim,
                                int32_t loss_kind, const float* params, const int64_t* offsets, const float* x, const void* y,
                                float* workspace, float* y_hat, float* loss_dev, int64_t max_rows, void* stream) {
  return mfm::predict_klef(T, N, D, h, zy, fy, output_dim, loss_kind, params, offsets, x, y, workspace, y_hat, loss_dev, max_rows,
                           (hipStream_t)stream);
}
