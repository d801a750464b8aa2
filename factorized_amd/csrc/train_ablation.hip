// One training step of the ablation M_D without the optimizer (include/mfm_hip.h, mfm_train_ablation_d): the label loss and its
// gradient with respect to all 32 parameter tensors -- the `train` block of the reference's train_mfm_ablation for the purely
// discriminative class: three own-modality encoders, three z -> f MLPs, one linear head; no decoders, no MMD, no KL.
//   z_m = encoder_m.fc1(h_T,m), f_m = relu(fc2(drop(relu(fc1(z_m))))) for m in l, a, v; y_hat = fs_to_y([f_l | f_a | f_v])
// Per row chunk, on one stream:
//   1. the three input projections on their column ranges of x as ONE grouped GEMM (gemm_group_launch) into gate records;
//   2. ONE forward recurrence launch for the three encoders with the BPTT record kept (the path of mfm_lstm_seq_fwd);
//   3. train_d_head_kernel, ONE launch over row tiles: a workgroup stays on chip from h_T to d h_T -- the three fc1, the MLPs
//      (dropout masks from rng_uniform), the head, the row's loss contribution, d y_hat and straight back through all ten
//      linears, whose inputs and gates are still in LDS.  It stores y_hat, d h_T,m, one loss contribution per row and ONE
//      partial of the ten weight / bias gradients per workgroup, then draws the launch's arrival ticket.  The workgroup that
//      draws the LAST ticket adds the partials tile by tile in a fixed order and writes (or adds to) the gradients, adds the
//      loss contributions in fp64 in a fixed order onto the running sum, writes the mean behind the last chunk and puts the
//      ticket back to 0;
//   4. ONE BPTT launch for the three encoders with dh_ext = the stored d h_T,m (the path of mfm_lstm_seq_bwd);
//   5. ONE grouped GEMM for dW_ih, dW_hh (T > 1) and both bias gradients of the three encoders, unsplit along K: one store or
//      one add per element.
// Nobody waits or spins, and no float atomic meets another on a result: loss and gradients are bit-identical from run to run.
// A row's arithmetic does not depend on its place in a tile or a chunk.  The head kernel's products are at most 128 wide on 1
// or 4 rows: it is bound by the latency of its twenty dependent layers (a barrier and an L2 round trip for the weights each),
// not by arithmetic -- quads of lanes per output and fp32 FMAs, as the latent row kernels, not the MFMA.
#include "infer_dev.h"
#include "internal.h"

namespace mfm {

#define TRD_MODS 3
#define TRD_MOD_PTRS 10      // per modality: 4 of the LSTM cell, 2 of the encoder's fc1, 4 of z<m>_to_f<m>
#define TRD_NPARAM (TRD_MODS * TRD_MOD_PTRS + 2)
#define TRD_NLIN 10          // linears of the head kernel: 3 m + {0 encoder fc1, 1 z->f fc1, 2 z->f fc2}; 9 fs_to_y
#define TRD_THREADS 1024

struct TrdLin { const float* w; const float* b; float* gw; float* gb; int K, N, poff, pad_; };      // poff: its weights' first float in a partial (bias behind)
struct TrdMod {
  const float* hT; float* dh; float* mask;     // this chunk's h_{T-1} [n, Hp], d h_T [n, z], dropout scales [n, f] (null: identity)
  float p, scale;                              // dropout probability (0: identity) and 1 / (1 - p)
  int z, f, Hp, col;                           // col: first column of f_m in the concatenated row
  int o_h, o_z, o_a, o_d1, o_dz, o_dh;         // LDS offsets in units of R floats: h_T, z, the MLP's hidden layer, and the gradients
};
struct TrdHeadDev {
  TrdLin lin[TRD_NLIN];
  TrdMod m[TRD_MODS];
  float* y_hat; const void* y;                 // this chunk's rows [n, od] and labels
  float* rowloss; float* partial; float* ones; // workspace: one contribution per row, one partial per workgroup, T * n ones
  double* acc; int* ticket; float* loss;
  const unsigned long long* tick;              // optional device word added to the seed
  unsigned long long seed;
  double inv;                                  // 1 / (N od) (L1) or 1 / N (CE): the WHOLE split
  int64_t row0;                                // the chunk's first row in the split (the masks are keyed by it)
  int n, T, ftot, od, psize, loss_kind, first, last, store;
  int o_f, o_d2, o_y, o_dy, o_flag;            // LDS: the f row, its gradient, y_hat, d y_hat (units of R floats); the flag (floats)
};

// dx[k][r] = gate(k, r, sum_c W[c][k] dy[c][r]): the transposed product of the backward.  A quad of lanes per input column k,
// lane q takes the output rows c = q + 4 j of W [N, K]; a wave reads 16 consecutive floats of four rows
template <int R, class G>
__device__ __forceinline__ void dense_rows_t(const float* __restrict__ W, const int K, const int N, const float* dy, float* dx, G gate) {
  const int tid = threadIdx.x, nq = blockDim.x >> 2, q = tid & 3;
  for (int k = tid >> 2; k < K; k += nq) {
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0f;
    for (int c = q; c < N; c += 4) {
      const float wv = W[(int64_t)c * K + k];
      const RowVec<R> yv = ld_rows<R>(dy + c * R);
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = fmaf(wv, yv.v[r], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float v = acc[r];
      v += dpp_f<DPP_QUAD_XOR1>(v);
      v += dpp_f<DPP_QUAD_XOR2>(v);
      if (q == 0) dx[k * R + r] = gate(k, r, v);
    }
  }
  lds_barrier();
}

// this workgroup's share of a linear's gradients: dW[c][k] = sum_r dy[c][r] in[k][r], db[c] = sum_r dy[c][r], into its partial
template <int R>
__device__ __forceinline__ void partial_products(const TrdLin& L, const float* dy, const float* in, float* part, const int tid) {
  const int K = L.K, NK = L.N * L.K;
  if (L.gw)
    for (int e = tid; e < NK; e += TRD_THREADS) {
      const int c = e / K, k = e - c * K;
      const RowVec<R> a = ld_rows<R>(dy + c * R), b = ld_rows<R>(in + k * R);
      float s = 0.0f;
#pragma unroll
      for (int r = 0; r < R; ++r) s = fmaf(a.v[r], b.v[r], s);
      __hip_atomic_store(part + L.poff + e, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  if (L.gb)
    for (int c = tid; c < L.N; c += TRD_THREADS) {
      const RowVec<R> a = ld_rows<R>(dy + c * R);
      float s = 0.0f;
#pragma unroll
      for (int r = 0; r < R; ++r) s += a.v[r];
      __hip_atomic_store(part + L.poff + NK + c, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// count floats of every workgroup's partial from `off` on, added tile by tile in a fixed order (four running sums over the
// tiles t = 0, 1, 2, 3 mod 4, then (s0 + s1) + (s2 + s3)) and stored to, or added to, g
__device__ __forceinline__ void reduce_partials(const float* part, const int64_t psize, const int tiles, const int off, const int count,
                                                float* g, const bool store, const int tid) {
  for (int e = tid; e < count; e += TRD_THREADS) {
    const float* p = part + off + e;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    int t = 0;
    for (; t + 4 <= tiles; t += 4) {
      s0 += __hip_atomic_load(p + (t + 0) * psize, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s1 += __hip_atomic_load(p + (t + 1) * psize, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s2 += __hip_atomic_load(p + (t + 2) * psize, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s3 += __hip_atomic_load(p + (t + 3) * psize, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (t < tiles) s0 += __hip_atomic_load(p + (t + 0) * psize, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t + 1 < tiles) s1 += __hip_atomic_load(p + (t + 1) * psize, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t + 2 < tiles) s2 += __hip_atomic_load(p + (t + 2) * psize, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const float s = (s0 + s1) + (s2 + s3);
    g[e] = store ? s : g[e] + s;
  }
}

template <int R>
__global__ __launch_bounds__(TRD_THREADS) void train_d_head_kernel(const TrdHeadDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, tile = blockIdx.x, b0 = tile * R, n = P.n;
  const int ftot = P.ftot, od = P.od;
  float* fcat = lds + P.o_f * R;
  float* d2 = lds + P.o_d2 * R;
  float* yh = lds + P.o_y * R;
  float* dy = lds + P.o_dy * R;
  // ---- forward: h_T of the three encoders into LDS (rows beyond n: zeros), then the three chains
#pragma unroll 1
  for (int m = 0; m < TRD_MODS; ++m) {
    const TrdMod& M = P.m[m];
    float* out = lds + M.o_h * R;
    for (int e = tid; e < M.z * R; e += TRD_THREADS) {
      const int r = e / M.z, k = e - r * M.z;
      out[k * R + r] = (b0 + r < n) ? M.hT[(int64_t)(b0 + r) * M.Hp + k] : 0.0f;
    }
  }
  lds_barrier();
  const unsigned long long seed = P.seed + (P.tick ? P.tick[0] : 0ull);
#pragma unroll 1
  for (int m = 0; m < TRD_MODS; ++m) {
    const TrdMod& M = P.m[m];
    const TrdLin* L = P.lin + 3 * m;
    float* zz = lds + M.o_z * R;
    float* a1 = lds + M.o_a * R;
    dense_rows<R>(L[0].w, L[0].b, M.z, M.z, lds + M.o_h * R, zz, false);
    dense_rows<R>(L[1].w, L[1].b, M.z, M.f, zz, a1, true);
    if (M.mask) {
      // the dropout scale of (site m, row, column): 0 or 1 / (1 - p), kept for the caller in the workspace
      for (int e = tid; e < M.f * R; e += TRD_THREADS) {
        const int r = e / M.f, o = e - r * M.f;
        const uint64_t idx = ((uint64_t)m << 40) + (uint64_t)(P.row0 + b0 + r) * (uint64_t)M.f + (uint64_t)o;
        const float mk = (rng_uniform(seed, idx) < M.p) ? 0.0f : M.scale;
        a1[o * R + r] *= mk;
        if (b0 + r < n) M.mask[(int64_t)(b0 + r) * M.f + o] = mk;
      }
      lds_barrier();
    }
    dense_rows<R>(L[2].w, L[2].b, M.f, M.f, a1, fcat + M.col * R, true);
  }
  const TrdLin& LY = P.lin[TRD_NLIN - 1];
  dense_rows<R>(LY.w, LY.b, ftot, od, fcat, yh, false);
  store_rows<R>(yh, P.y_hat, od, b0, n, tid);
  // ---- a row's loss contribution and d y_hat in a fixed order by one lane; rows beyond n: zeros, and so everything behind them
  if (tid < R) {
    const int row = b0 + tid;
    if (row < n) {
      float part = 0.0f;
      if (P.loss_kind == 0) {
        const float* yt = reinterpret_cast<const float*>(P.y) + (int64_t)row * od;
        const float g = (float)P.inv;
        for (int o = 0; o < od; ++o) {
          const float d = yh[o * R + tid] - yt[o];
          part += fabsf(d);
          dy[o * R + tid] = d > 0.0f ? g : (d < 0.0f ? -g : 0.0f);
        }
      } else {
        const int64_t lab = reinterpret_cast<const int64_t*>(P.y)[row];
        float mx = yh[tid];
        for (int o = 1; o < od; ++o) mx = fmaxf(mx, yh[o * R + tid]);
        float se = 0.0f;
        for (int o = 0; o < od; ++o) se += expf(yh[o * R + tid] - mx);
        const int lc = (int)min(max(lab, (int64_t)0), (int64_t)(od - 1));      // (a label outside [0, od) must not index outside LDS)
        part = (logf(se) + mx) - yh[lc * R + tid];
        const float g = (float)P.inv, rs = 1.0f / se;
        for (int o = 0; o < od; ++o) dy[o * R + tid] = (expf(yh[o * R + tid] - mx) * rs - (o == lc ? 1.0f : 0.0f)) * g;
      }
      __hip_atomic_store(P.rowloss + row, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      for (int o = 0; o < od; ++o) dy[o * R + tid] = 0.0f;
    }
  }
  lds_barrier();
  // ---- backward: the head, then the three chains down to d h_T
  dense_rows_t<R>(LY.w, ftot, od, dy, d2, [&](int k, int r, float v) { return fcat[k * R + r] > 0.0f ? v : 0.0f; });
#pragma unroll 1
  for (int m = 0; m < TRD_MODS; ++m) {
    const TrdMod& M = P.m[m];
    const TrdLin* L = P.lin + 3 * m;
    const float* a1 = lds + M.o_a * R;
    float* d1 = lds + M.o_d1 * R;
    float* dz = lds + M.o_dz * R;
    float* dh = lds + M.o_dh * R;
    const float sc = M.mask ? M.scale : 1.0f;
    // (a1 > 0 exactly where the ReLU passed and the mask kept: the gate of both, the kept scale is the same for all of them)
    dense_rows_t<R>(L[2].w, M.f, M.f, d2 + M.col * R, d1, [&](int k, int r, float v) { return a1[k * R + r] > 0.0f ? v * sc : 0.0f; });
    dense_rows_t<R>(L[1].w, M.z, M.f, d1, dz, [](int, int, float v) { return v; });
    dense_rows_t<R>(L[0].w, M.z, M.z, dz, dh, [](int, int, float v) { return v; });
    store_rows<R>(dh, M.dh, M.z, b0, n, tid);
  }
  // ---- this workgroup's partial of the ten weight / bias gradients (a frozen tensor: skipped), and its share of the ones
  float* part = P.partial + (int64_t)tile * P.psize;
#pragma unroll 1
  for (int m = 0; m < TRD_MODS; ++m) {
    const TrdMod& M = P.m[m];
    const TrdLin* L = P.lin + 3 * m;
    partial_products<R>(L[0], lds + M.o_dz * R, lds + M.o_h * R, part, tid);
    partial_products<R>(L[1], lds + M.o_d1 * R, lds + M.o_z * R, part, tid);
    partial_products<R>(L[2], d2 + M.col * R, lds + M.o_a * R, part, tid);
  }
  partial_products<R>(LY, dy, fcat, part, tid);
  const int ones_end = min((b0 + R) * P.T, n * P.T);
  for (int e = b0 * P.T + tid; e < ones_end; e += TRD_THREADS) P.ones[e] = 1.0f;
  // ---- the launch's arrival ticket (the pattern of ablation_encode_kernel): every wave's stores above have been acknowledged in
  // front of the barrier, the draw's release comes behind it; agent scope on the stores, the draw and the loads below
  int* flag = reinterpret_cast<int*>(lds + P.o_flag);
  const int tiles = (n + R - 1) / R;
  sync_stores();
  if (tid == 0) flag[0] = __hip_atomic_fetch_add(P.ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (flag[0] != tiles - 1) return;
  // ---- the last arriver: every other workgroup's partial and contributions were stored in front of its draw
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const bool store = P.store != 0;
#pragma unroll 1
  for (int l = 0; l < TRD_NLIN; ++l) {
    const TrdLin& L = P.lin[l];
    const int NK = L.N * L.K;
    if (L.gw) reduce_partials(P.partial, P.psize, tiles, L.poff, NK, L.gw, store, tid);
    if (L.gb) reduce_partials(P.partial, P.psize, tiles, L.poff + NK, L.N, L.gb, store, tid);
  }
  if (tid >= 64) return;
  // the chunk's loss contributions in fp64: lane l takes rows l, l + 64, ... ascending, then one fixed butterfly; the running sum
  // of the chunks so far is carried (the launches of a call are stream-ordered), the mean written behind the last chunk
  double s = 0.0;
  for (int i = tid; i < n; i += 64) s += (double)__hip_atomic_load(P.rowloss + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) s += __shfl_xor(s, w, 64);
  if (tid == 0) {
    if (!P.first) s += __hip_atomic_load(P.acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(P.acc, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (P.last) P.loss[0] = (float)(s * P.inv);
    __hip_atomic_store(P.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------- host
struct TrdSizes { int z[TRD_MODS], fm[TRD_MODS], dm[TRD_MODS], od, D, ftot, psize; };
// false: a size below 1
static bool trd_sizes(const int32_t* sz, TrdSizes& S) {
  if (!sz) return false;
  for (int i = 0; i < 12; ++i)
    if (sz[i] < 1) return false;
  for (int m = 0; m < TRD_MODS; ++m) { S.z[m] = sz[m]; S.fm[m] = sz[4 + m]; S.dm[m] = sz[8 + m]; }
  S.od = sz[11];
  S.D = S.dm[0] + S.dm[1] + S.dm[2];
  S.ftot = S.fm[0] + S.fm[1] + S.fm[2];
  int64_t p = (int64_t)S.od * S.ftot + S.od;
  for (int m = 0; m < TRD_MODS; ++m) {
    const int64_t z = S.z[m], f = S.fm[m];
    p += (z * z + z) + (f * z + f) + (f * f + f);      // the encoder's fc1, z -> f fc1, fc2: weights and bias each
  }
  if (p >= ((int64_t)1 << 30)) return false;
  S.psize = (int)up4(p);
  return true;
}

static int trd_tile_rows(int64_t rows) { return gen_tile_rows(TRD_MODS, (int)std::min<int64_t>(rows, INT32_MAX)); }

// the workspace, in this order (every part a multiple of 4 floats; include/mfm_hip.h states it term by term)
struct TrdLayout { int64_t gates, hs, cs, dh, mask, part, row, ones, tail, total; };
static TrdLayout trd_layout(int64_t T, int64_t N, const TrdSizes& S, int64_t max_rows) {
  const int64_t rows = gen_rows(N, max_rows);
  int64_t hp = 0, zs = 0;
  for (int m = 0; m < TRD_MODS; ++m) { hp += hp_of(S.z[m]); zs += up4(rows * S.z[m]); }
  TrdLayout o;
  o.gates = rows < N ? up4(T * rows * S.D) : 0;      // (in front: the chunk's copy of x)
  o.hs = o.gates + rows * T * 4 * hp;
  o.cs = o.hs + rows * T * hp;
  o.dh = o.cs + rows * T * hp;
  o.mask = o.dh + zs;
  o.part = o.mask + up4(rows * S.ftot);
  o.row = o.part + (rows + trd_tile_rows(rows) - 1) / trd_tile_rows(rows) * S.psize;
  o.ones = o.row + up4(rows);
  o.tail = o.ones + up4(rows * T);
  o.total = o.tail + 4;
  return o;
}

static int train_ablation_d(int T, int64_t N, const int32_t* sz, int loss_kind, int train, const float* p_drop, uint64_t seed,
                            uint64_t call, const unsigned long long* tick, const float* const* prm, float* const* grd, int accumulate,
                            const float* x, const void* y, float* ws, float* y_hat, float* loss, int64_t max_rows, hipStream_t stream) {
  static const char* who = "train ablation d";
  MFM_REQUIRE(sz && prm && grd && p_drop && x && y && ws && y_hat && loss,
              "%s: bad arguments (sizes, parameter and gradient tables, dropout table, x, labels, workspace, y_hat and loss must not be null)", who);
  int rc = infer_check_sizes(who, T, N, sz);
  if (rc != MFM_OK) return rc;
  if ((rc = infer_check_loss_kind(who, loss_kind)) != MFM_OK) return rc;
  if ((rc = infer_check_rows(who, N, max_rows)) != MFM_OK) return rc;
  MFM_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate = %d (0 or 1)", who, accumulate);
  MFM_REQUIRE(train == 0 || train == 1, "%s: train = %d (0 or 1)", who, train);
  for (int m = 0; m < TRD_MODS; ++m)
    MFM_REQUIRE(p_drop[m] >= 0.0f && p_drop[m] < 1.0f, "%s: dropout probability %d is %g (in [0, 1))", who, m, (double)p_drop[m]);
  MFM_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)ws & 15) == 0, "%s: x must be 4-byte aligned, the workspace 16-byte aligned", who);
  MFM_REQUIRE((((uintptr_t)y_hat | (uintptr_t)loss) & 3) == 0 && ((uintptr_t)y & (loss_kind == 0 ? 3 : 7)) == 0 && ((uintptr_t)tick & 7) == 0,
              "%s: y_hat, loss, the labels or the tick word are misaligned", who);
  for (int i = 0; i < TRD_NPARAM; ++i) {
    const int m = i / TRD_MOD_PTRS, j = i % TRD_MOD_PTRS;
    MFM_REQUIRE(prm[i], "%s: parameter %d is null", who, i);
    const bool lstm_w = m < TRD_MODS && j < 2;
    MFM_REQUIRE(((uintptr_t)prm[i] & (lstm_w ? 15 : 3)) == 0, "%s: parameter %d is misaligned (LSTM weights 16 bytes, the rest 4)", who, i);
    MFM_REQUIRE(((uintptr_t)grd[i] & 3) == 0, "%s: gradient %d is misaligned", who, i);
  }
  TrdSizes S;
  MFM_REQUIRE(trd_sizes(sz, S), "%s: the ten head linears together are too large", who);
  for (int m = 0; m < TRD_MODS; ++m) {
    if ((rc = infer_check_resident(who, S.z[m])) != MFM_OK) return rc;
    if (S.fm[m] > MFM_SEQ_MAX_RESIDENT_H) {
      set_error("%s: f size %d of modality %d is beyond the on-chip head (at most %d)", who, S.fm[m], m, MFM_SEQ_MAX_RESIDENT_H);
      return MFM_ERR_UNSUPPORTED;
    }
  }
  const int rows = (int)gen_rows(N, max_rows);
  const int R = trd_tile_rows(rows);
  // the LDS of a head workgroup, in units of R floats, every part a multiple of 4: per modality h_T, z, d z, d h_T (z each), the
  // MLP's hidden layer and its gradient (f each); the f row and its gradient; y_hat and d y_hat; 4 floats for the ticket's answer
  TrdHeadDev P;
  memset(&P, 0, sizeof(P));
  int64_t o = 0;
  int maxhp = 16;
  for (int m = 0; m < TRD_MODS; ++m) {
    TrdMod& M = P.m[m];
    M.z = S.z[m]; M.f = S.fm[m]; M.Hp = (int)hp_of(S.z[m]);
    maxhp = std::max(maxhp, M.Hp);
    const int zu = (int)up4(M.z), fu = (int)up4(M.f);
    M.o_h = (int)o; o += zu; M.o_z = (int)o; o += zu; M.o_dz = (int)o; o += zu; M.o_dh = (int)o; o += zu;
    M.o_a = (int)o; o += fu; M.o_d1 = (int)o; o += fu;
  }
  P.o_f = (int)o; o += up4(S.ftot); P.o_d2 = (int)o; o += up4(S.ftot);
  P.o_y = (int)o; o += up4(S.od); P.o_dy = (int)o; o += up4(S.od);
  const int64_t lds_floats = o * R + 4;
  if (lds_floats * 4 > 160 * 1024) {
    set_error("%s: a head row of output_dim = %d beside fl + fa + fv = %d (%d rows per workgroup, %lld bytes of LDS) exceeds the 160 KB of a CU",
              who, S.od, S.ftot, R, (long long)(lds_floats * 4));
    return MFM_ERR_UNSUPPORTED;
  }
  P.o_flag = (int)(o * R);
  const size_t lds_bytes = lds_bytes_of((size_t)lds_floats);
  if ((rc = infer_check_chunk(who, rows, T, std::max(S.D, 4 * maxhp), "projection")) != MFM_OK) return rc;
  const int64_t tiles_max = cdiv(rows, R);
  MFM_REQUIRE(tiles_max * S.psize < ((int64_t)1 << 40), "%s: a chunk of %d rows is too large; pass a row cap", who, rows);

  // ---- everything that does not depend on the chunk
  const TrdLayout lay = trd_layout(T, N, S, max_rows);
  const bool chunked = rows < N;
  float* xc = ws;
  SeqDev seq[TRD_MODS];
  MfmSeqDesc sd[TRD_MODS];
  memset(sd, 0, sizeof(sd));
  int poff = 0;
  for (int m = 0, fcol = 0; m < TRD_MODS; ++m) {
    const float* const* p = prm + m * TRD_MOD_PTRS;
    float* const* g = grd + m * TRD_MOD_PTRS;
    seq_fill(seq[m], p[0], p[1], p[2], p[3], S.z[m], 0);
    TrdMod& M = P.m[m];
    M.col = fcol; fcol += S.fm[m];
    M.p = p_drop[m]; M.scale = 1.0f / (1.0f - p_drop[m]);
    const int K[3] = {S.z[m], S.z[m], S.fm[m]}, Nn[3] = {S.z[m], S.fm[m], S.fm[m]};
    for (int l = 0; l < 3; ++l) {
      TrdLin& L = P.lin[3 * m + l];
      L.w = p[4 + 2 * l]; L.b = p[5 + 2 * l]; L.gw = g[4 + 2 * l]; L.gb = g[5 + 2 * l];
      L.K = K[l]; L.N = Nn[l]; L.poff = poff; poff += L.N * L.K + L.N;
    }
  }
  {
    TrdLin& L = P.lin[TRD_NLIN - 1];
    L.w = prm[30]; L.b = prm[31]; L.gw = grd[30]; L.gb = grd[31];
    L.K = S.ftot; L.N = S.od; L.poff = poff;
  }
  P.rowloss = ws + lay.row; P.partial = ws + lay.part; P.ones = ws + lay.ones;
  P.acc = reinterpret_cast<double*>(ws + lay.tail);      // (a multiple of 4 floats from a 16-byte aligned base)
  P.ticket = reinterpret_cast<int*>(ws + lay.tail + 2);
  P.loss = loss; P.tick = tick;
  P.seed = seed + 0x9E3779B97F4A7C15ull * call;
  P.inv = inv_label_count(loss_kind, N, S.od);
  P.T = T; P.ftot = S.ftot; P.od = S.od; P.psize = S.psize; P.loss_kind = loss_kind;
  // the ticket word and the running sum start at 0 (the workspace's contents are arbitrary, and a call that ended in an error
  // between two launches may have left arrivals behind): cleared by the first projection launch of the call
  ZeroSpans zs;
  memset(&zs, 0, sizeof(zs));
  zs.ptr[0] = ws + lay.tail; zs.n[0] = 4;

  for (int64_t n0 = 0; n0 < N; n0 += rows) {
    const int n = (int)std::min<int64_t>(rows, N - n0);
    const bool first = n0 == 0, store = first && !accumulate;
    // a chunk of a longer split: its rows of x as one [T n, D] matrix (the weight-gradient products walk all T n rows at once)
    const float* xs = x;
    if (chunked) {
      MFM_HIP_CHECK(hipMemcpy2DAsync(xc, (size_t)n * S.D * sizeof(float), x + n0 * S.D, (size_t)N * S.D * sizeof(float), (size_t)n * S.D * sizeof(float),
                                     (size_t)T, hipMemcpyDeviceToDevice, stream));
      xs = xc;
    }
    // ---- 1. the projections
    float* gates = ws + lay.gates;
    float* hs = ws + lay.hs;
    float* cs = ws + lay.cs;
    float* dh = ws + lay.dh;
    float* mask = ws + lay.mask;
    MfmGemmDesc g[4 * TRD_MODS];
    memset(g, 0, sizeof(g));
    for (int m = 0, col = 0; m < TRD_MODS; ++m) {
      SeqDev& s = seq[m];
      TrdMod& M = P.m[m];
      s.gates = gates; s.hs = hs; s.cs = cs;
      xproj_desc(g[m], s, xs + col, S.D, S.dm[m], T * n, gates);
      MfmSeqDesc& d = sd[m];
      d.gates = gates; d.hs = hs; d.cs = cs; d.w_hh = s.w_hh; d.h = s.h;
      d.dh_ext = dh; d.ld_dh = s.h;
      M.hT = hs + (int64_t)(T - 1) * n * s.Hp; M.dh = dh;
      M.mask = (train && p_drop[m] > 0.0f) ? mask : nullptr;
      gates += (int64_t)rows * T * 4 * s.Hp; hs += (int64_t)rows * T * s.Hp; cs += (int64_t)rows * T * s.Hp;
      dh += up4((int64_t)rows * s.h); mask += (int64_t)rows * S.fm[m];
      col += S.dm[m];
    }
    if ((rc = gemm_group_launch(g, TRD_MODS, stream, first ? &zs : nullptr)) != MFM_OK) return rc;
    // ---- 2. the recurrences, the record kept
    if ((rc = mfm_lstm_seq_fwd(sd, TRD_MODS, T, n, stream)) != MFM_OK) return rc;
    // ---- 3. the head
    P.n = n; P.row0 = n0;
    P.y_hat = y_hat + n0 * S.od;
    P.y = labels_at(y, loss_kind, n0, S.od);
    P.first = first; P.last = n0 + n == N; P.store = store;
    const int tiles = cdiv(n, R);
    rc = (R == 1) ? seq_launch_kernel(train_d_head_kernel<1>, "train_d_head_kernel", dim3(tiles), dim3(TRD_THREADS), lds_bytes, stream, nullptr, P)
                  : seq_launch_kernel(train_d_head_kernel<4>, "train_d_head_kernel", dim3(tiles), dim3(TRD_THREADS), lds_bytes, stream, nullptr, P);
    if (rc != MFM_OK) return rc;
    // ---- 4. the BPTT: the gate records become dA in place
    if ((rc = mfm_lstm_seq_bwd(sd, TRD_MODS, T, n, stream)) != MFM_OK) return rc;
    // ---- 5. the encoders' weight gradients, unsplit along K: one store (or one add) per element
    memset(g, 0, sizeof(g));
    int cnt = 0;
    for (int m = 0, col = 0; m < TRD_MODS; ++m) {
      const SeqDev& s = seq[m];
      float* const* gp = grd + m * TRD_MOD_PTRS;
      const int h = s.h, d = S.dm[m];
      auto base = [&](MfmGemmDesc& q, const float* a, int k) {
        q.a = a; q.a_sm = 1; q.a_sk = 4 * (int64_t)s.Hp; q.a_sz = s.Hp;
        q.m = h; q.k = k; q.batch = 4; q.split_k = 1; q.accumulate = store ? 0 : 1; q.alpha = 1.0f;
      };
      if (gp[0]) {
        MfmGemmDesc& q = g[cnt++];
        base(q, s.gates, T * n);
        q.b = xs + col; q.b_sk = S.D; q.b_sn = 1;
        q.c = gp[0]; q.ldc = d; q.c_sz = (int64_t)h * d; q.n = d; q.n_valid = d;
      }
      if (gp[1]) {
        if (T > 1) {
          MfmGemmDesc& q = g[cnt++];
          base(q, s.gates + (int64_t)n * 4 * s.Hp, (T - 1) * n);
          q.b = s.hs; q.b_sk = s.Hp; q.b_sn = 1;
          q.c = gp[1]; q.ldc = h; q.c_sz = (int64_t)h * h; q.n = h; q.n_valid = h;
        } else if (store) {
          MFM_HIP_CHECK(hipMemsetAsync(gp[1], 0, (size_t)4 * h * h * sizeof(float), stream));      // (no step feeds W_hh: exact zeros)
        }
      }
      if (gp[2] || gp[3]) {
        MfmGemmDesc& q = g[cnt++];
        base(q, s.gates, T * n);
        q.b = P.ones; q.b_sk = 1; q.b_sn = 1;
        q.c = gp[2] ? gp[2] : gp[3]; q.c2 = gp[2] ? gp[3] : nullptr; q.ldc = 1; q.c_sz = h; q.n = 1; q.n_valid = 1;
      }
      col += d;
    }
    if (cnt && (rc = gemm_group_launch(g, cnt, stream)) != MFM_OK) return rc;
  }
  return MFM_OK;
}

}  // namespace mfm

extern "C" int64_t mfm_train_ablation_d_workspace_floats(int32_t T, int64_t N, const int32_t* sizes, int64_t max_rows) {
  mfm::TrdSizes S;
  if (T < 1 || N < 1 || N >= ((int64_t)1 << 24) || max_rows < 0 || !mfm::trd_sizes(sizes, S)) return 0;
  return mfm::trd_layout(T, N, S, max_rows).total;
}

extern "C" int64_t mfm_train_ablation_d_mask_offset(int32_t T, int64_t N, const int32_t* sizes, int64_t max_rows) {
  mfm::TrdSizes S;
  if (T < 1 || N < 1 || N >= ((int64_t)1 << 24) || max_rows < 0 || !mfm::trd_sizes(sizes, S)) return 0;
  return mfm::trd_layout(T, N, S, max_rows).mask;
}

extern "C" int mfm_train_ablation_d_tile_rows(int64_t N, int64_t max_rows, int32_t* tile_rows) {
  if (N < 1 || max_rows < 0 || !tile_rows) {
    mfm::set_error("train ablation d tile rows: bad arguments (N %lld, row cap %lld)", (long long)N, (long long)max_rows);
    return MFM_ERR_ARG;
  }
  tile_rows[0] = mfm::trd_tile_rows(mfm::gen_rows(N, max_rows));
  return MFM_OK;
}

extern "C" int mfm_train_ablation_d(int32_t T, int64_t N, const int32_t* sizes, int32_t loss_kind, int32_t train, const float* p_drop,
                                    uint64_t seed, uint64_t call, const uint64_t* tick, const float* const* params, float* const* grads,
                                    int32_t accumulate, const float* x, const void* y, float* workspace, float* y_hat, float* loss,
                                    int64_t max_rows, void* stream) {
  return mfm::train_ablation_d(T, N, sizes, loss_kind, train, p_drop, seed, call, reinterpret_cast<const unsigned long long*>(tick), params,
                               grads, accumulate, x, y, workspace, y_hat, loss, max_rows, (hipStream_t)stream);
}
