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
#include "infer_dev.h"

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
  store_rows<R>(in, P.y_hat, od, b0, P.n, tid);
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

// floats: the x-projections of one row chunk, one loss partial per row (a one-row tile each at most), the ticket word (+ pad)
static int64_t predict_ws_floats(int64_t T, int64_t N, int64_t h, int64_t max_rows) {
  return gen_rows(N, max_rows) * T * 4 * hp_of(h) + N + 4;
}

template <int R>
static int predict_launch_r(const PredictDev& P, int grid, int threads, size_t lds_bytes, hipStream_t stream) {
  return infer_launch_hk4("predict klef", "predict_klef_kernel", P.seq, [](auto kk) { return predict_klef_kernel<decltype(kk)::value, R>; },
                          P, grid, threads, lds_bytes, stream);
}

static int predict_klef(int T, int64_t N, int D, int h, int zy, int fy, int od, int loss_kind, const float* params,
                        const int64_t* offs, const float* x, const void* y, float* ws, float* y_hat, float* loss_dev,
                        int64_t max_rows, hipStream_t stream) {
  static const char* who = "predict klef";
  MFM_REQUIRE(T >= 1 && N >= 1 && D >= 1 && h >= 1 && zy >= 1 && fy >= 1 && od >= 1, "%s: sizes must be positive (T %d, N %lld, D %d, h %d, zy %d, fy %d, output_dim %d)",
              who, T, (long long)N, D, h, zy, fy, od);
  int rc = infer_check_loss_kind(who, loss_kind);
  if (rc != MFM_OK) return rc;
  MFM_REQUIRE(params && offs && x && ws && y_hat, "%s: bad arguments (params, offsets, x, workspace and y_hat must not be null)", who);
  if ((rc = infer_check_aligned(who, params, x, ws)) != MFM_OK) return rc;
  if ((rc = infer_check_rows(who, N, max_rows)) != MFM_OK) return rc;
  if ((rc = infer_check_offsets(who, offs, 4 + 2 * PRED_LAYERS, 4 + 2 * PRED_LAYERS)) != MFM_OK) return rc;
  const int maxw = std::max(std::max(h, zy), std::max(fy, od));
  const int rows = (int)gen_rows(N, max_rows);
  const int R = gen_tile_rows(1, rows), Hp = round_up(h, 16);
  const size_t lds_bytes = lds_bytes_of(enc_lds_floats(h, R, 2, maxw));      // (the heads ping-pong between two activations)
  if ((rc = infer_check_resident(who, h)) != MFM_OK) return rc;
  if ((rc = infer_check_lds(who, lds_bytes, maxw, R, h)) != MFM_OK) return rc;
  if ((rc = infer_check_chunk(who, rows, T, std::max(D, 4 * Hp), "projection")) != MFM_OK) return rc;

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
  P.seq.gates = gates;
  seq_fill(P.seq, params + offs[0], params + offs[1], params + offs[2], params + offs[3], h, 0);
  const int K[PRED_LAYERS] = {h, h, zy, fy, fy, fy}, Nn[PRED_LAYERS] = {h, zy, fy, fy, fy, od};
  const int relu[PRED_LAYERS] = {0, 0, 1, 1, 1, 0};
  for (int l = 0; l < PRED_LAYERS; ++l) {
    P.w[l] = params + offs[4 + 2 * l]; P.b[l] = params + offs[5 + 2 * l];
    P.K[l] = K[l]; P.N[l] = Nn[l]; P.relu[l] = relu[l];
  }
  P.T = T; P.od = od; P.loss_kind = loss_kind; P.maxw = maxw;
  P.partials = partials; P.ticket = ticket; P.loss = with_loss ? loss_dev : nullptr;
  P.wg_total = wg_total;
  P.inv = (float)inv_label_count(loss_kind, N, od);
  const int threads = std::max(8 * Hp, 64);

  int wg_base = 0;
  for (int64_t n0 = 0; n0 < N; n0 += rows) {
    const int n = (int)std::min<int64_t>(rows, N - n0);
    // gates[t][i][g][u] = x[t][n0 + i] . W_ih[g h + u] + b_ih + b_hh; pad units u >= h exact zeros
    const bool whole = n == N;           // one chunk: the T * N rows of x are one matrix
    rc = gemm_group_each(whole ? 1 : T, stream, [&](int t, MfmGemmDesc& d) {
      xproj_desc(d, P.seq, x + ((int64_t)t * N + n0) * D, D, D, whole ? T * n : n, gates + (int64_t)t * n * 4 * Hp);
    });
    if (rc != MFM_OK) return rc;
    P.n = n;
    P.y = with_loss ? labels_at(y, loss_kind, n0, od) : nullptr;
    P.y_hat = y_hat + n0 * od;
    P.wg_base = wg_base;
    const int grid = cdiv(n, R);
    rc = (R == 1) ? predict_launch_r<1>(P, grid, threads, lds_bytes, stream) : predict_launch_r<4>(P, grid, threads, lds_bytes, stream);
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
