// Whole-sequence LSTM recurrence for SMALL batch tiles (latency regime): the kernels and launchers around the device bodies of
// lstm_seq_small_dev.h -- the plain multi-LSTM launches, the fold launches that also run the rows' latent chains (MFM_KL_EF), and
// the role-workgroup launches (input projections / weight gradients on the idle CUs, proj_role_dev.h / dw_role_dev.h).
#include "lstm_seq_small_dev.h"

namespace mfm {

#define MFM_SMALL_CASE(KK, BODY) case KK: BODY<KK, 4>(d, L.T, L.B, tile, lds); break;
#define MFM_SMALL_CASES(BODY) switch (d.hk4) { MFM_HK4_CASES(MFM_SMALL_CASE, BODY) default: break; }

template <bool BWD>
__global__ __launch_bounds__(1024) void lstm_seq_small_kernel(const SeqLaunch L) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int bid = blockIdx.x;
  MFM_SEQ_BLOCK_LSTM(L, bid, di)
  const SeqDev& d = L.d[di];
  const int tile = bid - d.block_begin;
  if (BWD) {
    MFM_SMALL_CASES(small_bwd_body)
  } else {
    MFM_SMALL_CASES(small_fwd_body)
  }
}

// Specialised launch for a fixed tuple of per-LSTM variants: with 4 bodies in the kernel instead of
// 16 the register allocator reaches single-variant quality (the 16-way switch spills ~80 VGPRs in the
// forward time loop, 4x slower).  The canonical MFM sizes (encoders 32/8/80/120, decoders 104/24/24)
// are pre-instantiated; any other size combination takes the generic kernel above.
// KS = 8 (backward, one-row tiles): 4 * Hp threads per workgroup, launched with at most 512 -> 256 VGPRs per thread for
// the doubled resident weights.
template <bool BWD, int R, int KS, int K0, int K1, int K2, int K3, int K4 = 0, int K5 = 0, bool BF = false>
__global__ __launch_bounds__(KS == 16 ? 1024 : 512) void lstm_seq_small_kernel4(const SeqLaunch L) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int bid = blockIdx.x;
  LSTAMP(BWD ? 3 : 1, 0);
  if constexpr (!BWD) {      // blocks behind the recurrence rows: this step's transposed-weight images (lstm_seq_dev.h)
    if (L.n_img > 0 && bid >= L.img_begin) { wt_img_write(L.img, L.n_img, bid - L.img_begin, L.n_img_blocks); LSTAMP(1, 15); return; }
  }
  MFM_SEQ_BLOCK_LSTM(L, bid, di)
  const SeqDev& d = L.d[di];
  const int tile = bid - d.block_begin;
  MFM_TUPLE6(if (BWD) small_bwd_body<KQ, R, KS>(d, L.T, L.B, tile, lds); else small_fwd_body<KQ, R, false, BF>(d, L.T, L.B, tile, lds);
             LSTAMP(BWD ? 3 : 1, 15); return)
}

// ---------------------------------------------------------------- host helpers the launchers share
static const int kEncHk4[4] = {8, 2, 20, 30};      // the canonical MFM_KL_EF encoders (h = 32 / 8 / 80 / 120) ...
static const int kDecHk4[3] = {26, 6, 6};          // ... and decoders (h = 104 / 24 / 24)

// L holds exactly the LSTMs of these hk4, in this order; kind 0: all encoders, 1: all decoders, -1: either
static bool seq_is_tuple(const SeqLaunch& L, const int* hk4, int n, int kind) {
  if (L.count != n) return false;
  for (int i = 0; i < n; ++i)
    if (L.d[i].hk4 != hk4[i] || (kind >= 0 && (L.d[i].is_dec != 0) != (kind == 1))) return false;
  return true;
}
// the latent stack runs as four chain workgroups per row of the same batch: what a launch that carries chains needs
static bool chain_rows_match(const LatentDev& LD, int B) { return LD.row_path && LD.nch == 4 && !LD.pre && LD.B == B; }
// LDS of a chain workgroup: the stage tables + the row's record (backward: + its gradient record)
static size_t chain_lds_bytes(const LatentDev& LD, bool bwd) {
  return (size_t)(bwd ? latent_bwd_grd_floats(LD.rec_size) + LD.rec_size : latent_fwd_lds_floats(LD.rec_size)) * sizeof(float);
}
// `rows` blocks per LSTM from block `first` on; returns the first block behind them
static int lay_out_blocks(SeqLaunch& L, int rows, int first = 0) {
  int total = first;
  for (int i = 0; i < L.count; ++i) { L.d[i].block_begin = total; total += rows; }
  return total;
}
// forward, one-row tiles: blocks behind the `total` recurrence rows write this step's weight images (L.img) -- the idle CUs, at
// most 64; no idle CU left: the writers still pay (they run in the launch's last round, ~2 us, against ~9 us of staging saved)
static int add_img_writers(SeqLaunch& L, int total) {
  const int idle = device_cus() - total;
  L.img_begin = total; L.n_img_blocks = idle >= 8 ? std::min(idle, 64) : 32;
  return total + L.n_img_blocks;
}

template <int R, int KS, int K0, int K1, int K2, int K3, int K4 = 0, int K5 = 0>
static bool try_launch4(const SeqLaunch& L, bool bwd, int total, int threads, size_t lds_bytes, hipStream_t stream, int* rc) {
  const int want[6] = {K0, K1, K2, K3, K4, K5};
  int n = 0;
  for (int i = 0; i < 6; ++i) if (want[i] > 0) n = i + 1;
  if (!seq_is_tuple(L, want, n, -1)) return false;
  *rc = seq_launch_kernel(bwd ? lstm_seq_small_kernel4<true, R, KS, K0, K1, K2, K3, K4, K5> : lstm_seq_small_kernel4<false, R, KS, K0, K1, K2, K3, K4, K5>,
                          bwd ? "lstm_seq_small_bwd_kernel4" : "lstm_seq_small_fwd_kernel4", dim3(total), dim3(threads), lds_bytes, stream, nullptr, L);
  return true;
}

template <int R>
static bool try_all(const SeqLaunch& L, bool bwd, int total, int threads, size_t lds_bytes, hipStream_t stream, int* err) {
  // (from 2 rounds of workgroups on, the launcher orders the LSTMs of a call widest first: lstm_seq.hip)
  return try_launch4<R, 16, 8, 2, 20, 30>(L, bwd, total, threads, lds_bytes, stream, err) ||     // MFM_KL_EF encoders
         try_launch4<R, 16, 30, 20, 8, 2>(L, bwd, total, threads, lds_bytes, stream, err) ||
         try_launch4<R, 16, 26, 6, 6, 0>(L, bwd, total, threads, lds_bytes, stream, err) ||      // decoders
         try_launch4<R, 16, 30, 0, 0, 0>(L, bwd, total, threads, lds_bytes, stream, err) ||      // single-LSTM launches
         try_launch4<R, 16, 26, 0, 0, 0>(L, bwd, total, threads, lds_bytes, stream, err) ||
         try_launch4<R, 16, 8, 0, 0, 0>(L, bwd, total, threads, lds_bytes, stream, err) ||
         // (round 6: h = 24 / 8 / 80 alone.  scripts/bench_seq_group.py used to time these through the generic 4-row kernel -- the
         //  "h = 24 costs what h = 104 costs" of the round-5 review was that kernel, not the one-row bodies the plan runs)
         try_launch4<R, 16, 6, 0, 0, 0>(L, bwd, total, threads, lds_bytes, stream, err) ||
         try_launch4<R, 16, 2, 0, 0, 0>(L, bwd, total, threads, lds_bytes, stream, err) ||
         try_launch4<R, 16, 20, 0, 0, 0>(L, bwd, total, threads, lds_bytes, stream, err) ||
         // MFM / MFM_KL on the module path (mfm_model.py::seq_group): encoders 32/8/80 + MFN LSTM 88, MFN 64/48
         try_launch4<R, 16, 8, 2, 20, 22>(L, bwd, total, threads, lds_bytes, stream, err) ||
         try_launch4<R, 16, 16, 12, 0, 0>(L, bwd, total, threads, lds_bytes, stream, err) ||
         // MFM / MFM_KL on the fused plan: all six LSTMs of the step (encoders 32/8/80, MFN 88/64/48) in one launch
         try_launch4<R, 16, 8, 2, 20, 22, 16, 12>(L, bwd, total, threads, lds_bytes, stream, err);
}

// backward, one-row tiles, 8 k-slices (4 * Hp threads): the pre-instantiated size tuples
static bool try_all_fat(const SeqLaunch& L, int total, int threads, size_t lds_bytes, hipStream_t stream, int* err) {
  return try_launch4<1, 8, 8, 2, 20, 30>(L, true, total, threads, lds_bytes, stream, err) ||
         try_launch4<1, 8, 26, 6, 6, 0>(L, true, total, threads, lds_bytes, stream, err) ||
         try_launch4<1, 8, 30, 0, 0, 0>(L, true, total, threads, lds_bytes, stream, err) ||
         try_launch4<1, 8, 26, 0, 0, 0>(L, true, total, threads, lds_bytes, stream, err) ||
         try_launch4<1, 8, 8, 0, 0, 0>(L, true, total, threads, lds_bytes, stream, err) ||
         try_launch4<1, 8, 8, 2, 20, 22>(L, true, total, threads, lds_bytes, stream, err) ||
         try_launch4<1, 8, 16, 12, 0, 0>(L, true, total, threads, lds_bytes, stream, err) ||
         try_launch4<1, 8, 8, 2, 20, 22, 16, 12>(L, true, total, threads, lds_bytes, stream, err);
}

// Fold launch (MFM_KL_EF at small batches): the workgroup of (encoder e, batch row b) also runs modality chain e of row
// b's latent stack -- forward right behind its last time step, backward ahead of its BPTT.  The four chains are
// independent inside the stack and map one to one onto the four encoders, so nothing is exchanged between workgroups:
// what used to be a launch boundary (~3 us) plus the chain kernel's cold prologue becomes a barrier.  One-row tiles
// and the canonical size tuple only; anything else keeps the separate launches.
template <bool BWD, int K0, int K1, int K2, int K3>
__global__ __launch_bounds__(1024) void lstm_seq_small_fold_kernel(const SeqLaunch L, const LatentDev LD, const float* __restrict__ params,
                                                                   float* __restrict__ grads) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int bid = blockIdx.x;
  if constexpr (!BWD) {      // blocks behind the recurrence rows: this step's transposed-weight images (lstm_seq_dev.h)
    if (L.n_img > 0 && bid >= L.img_begin) { wt_img_write(L.img, L.n_img, bid - L.img_begin, L.n_img_blocks); return; }
  }
  MFM_SEQ_BLOCK_LSTM(L, bid, di)
  const SeqDev& d = L.d[di];
  const int tile = bid - d.block_begin;          // == batch row (one-row tiles)
  if constexpr (BWD) {
    latent_bwd_row_body<false>(LD, params, grads, tile, di, lds);
    sync_stores();           // d h_T of this (row, encoder) is in memory (and the LDS is free) before the BPTT reads it
  }
  MFM_TUPLE4(if (BWD) small_bwd_body<KQ, 1, 16>(d, L.T, L.B, tile, lds); else small_fwd_body<KQ, 1>(d, L.T, L.B, tile, lds))
  if constexpr (!BWD) {
    sync_stores();           // every store of the last time step has been acknowledged: h_T of this row is readable
    latent_fwd_row_body<false>(LD, params, tile, di, lds, true);
  }
}

// Forward fold launch with projection role workgroups (proj_role_dev.h): blocks [0, n_role) produce the x-projections
// (and clear the launch's zero spans), blocks [n_role, n_role + 4 B) are the fold launch's (encoder, row) workgroups.
template <int K0, int K1, int K2, int K3>
__global__ __launch_bounds__(1024) void lstm_seq_small_foldproj_kernel(const SeqLaunch L, const LatentDev LD, const ProjRole PR,
                                                                       const float* __restrict__ params) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int bid = blockIdx.x;
  const unsigned epoch = ho_epoch(PR.epoch, PR.tick);
  LSTAMP(0, 0);
  if (bid < PR.n_role) { proj_role_body(L, PR, epoch, lds); LSTAMP(0, 15); return; }
  MFM_SEQ_BLOCK_LSTM(L, bid, di)
  const SeqDev& d = L.d[di];
  const int tile = bid - d.block_begin;
  const unsigned long long* pw = PR.words + PR.e[di].w_off;          // this encoder's columns of the projection words
  // PR.lat_pre (every encoder loads its weights straight into registers: no LDS weight panel): the chain's tables go to LDS NOW,
  // while the row waits for its first projections anyway; the recurrence's buffers lie behind the chain's region, and the chain
  // takes h_T from the recurrence's LDS buffer instead of reading it back from memory behind a store wait
  const bool pre = PR.lat_pre != 0;
  float* seq_lds = lds;
  if (pre) {
    latent_fwd_row_body<false>(LD, params, tile, di, lds, true, 1);
    seq_lds = lds + latent_fwd_lds_floats(LD.rec_size);
  }
  const float* h_lds = nullptr;
  MFM_TUPLE4(h_lds = small_fwd_body<KQ, 1, true>(d, L.T, L.B, tile, seq_lds, pw, epoch, PR.w_ld, PR.ctl))
  // the loss slots are cleared by the producers of t = 0: all of them have passed before this row's chain adds to them
  // (the four flag sets are requested together: one round trip)
  if (threadIdx.x < 64) {
    unsigned fv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) fv[e] = proj_flags_load(PR.flags + (int64_t)e * L.T * PROJ_ROLE_FLAGS, PR.e[e].ncb);
#pragma unroll
    for (int e = 0; e < 4; ++e) proj_flags_wait(PR.flags + (int64_t)e * L.T * PROJ_ROLE_FLAGS, fv[e], epoch, PR.e[e].ncb, PR.ctl);
  }
  LSTAMP(0, 9);
  if (pre) {
    LSTAMP(0, 8);
    // (its first barrier orders the flag wait above)
    latent_fwd_row_body<false>(LD, params, tile, di, lds, true, 2, h_lds, PR.lat_tail ? LD.tail_from : MFM_LAT_MAXSTAGES);
  } else {
    sync_stores();           // every store of the last time step has been acknowledged: h_T of this row is readable
    LSTAMP(0, 8);
    latent_fwd_row_body<false>(LD, params, tile, di, lds, true);
  }
  LSTAMP_W(0, 15);
}

// Backward fold launch with weight-gradient role workgroups (dw_role_dev.h): blocks [0, 4 B) are the fold launch's
// (encoder, row) workgroups, blocks [4 B, 4 B + n_role) run the table of weight-gradient blocks.
template <int K0, int K1, int K2, int K3>
__global__ __launch_bounds__(1024) void lstm_seq_small_folddw_kernel(const SeqLaunch L, const LatentDev LD, const DwRole DR,
                                                                     const float* __restrict__ params, float* __restrict__ grads) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int bid = blockIdx.x;
  const unsigned epoch = ho_epoch(DR.epoch, DR.tick);
  LSTAMP(4, 0);
  if (bid >= 4 * L.B) {
    // (the DwRole descriptor as it lies in the kernel-argument segment, behind L and LD: dw_role_dev.h reads it with per-lane indices)
    typedef __attribute__((address_space(4))) const char kchar;
    const char* kargs = (const char*)(kchar*)__builtin_amdgcn_kernarg_segment_ptr();
    dw_role_body(DR, epoch, lds, reinterpret_cast<const int*>(kargs + sizeof(SeqLaunch) + sizeof(LatentDev)));
    LSTAMP_W(4, 15);
    return;
  }
  // a plan whose status word is set (a hand-over of this or of an earlier step gave up: the forward's projections may be
  // garbage) must not train: the guard word of the gradient buffer makes the optimizer skip (and travels through the all-reduce)
  if (bid == 0 && threadIdx.x == 0 && DR.ctl.status && DR.ctl.poison && *DR.ctl.status != 0u)
    __hip_atomic_store(DR.ctl.poison, __builtin_nanf(""), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  MFM_SEQ_BLOCK_LSTM(L, bid, di)
  const SeqDev& d = L.d[di];
  const int tile = bid - d.block_begin;          // == batch row (one-row tiles)
  unsigned* stamp = DR.flags + (int64_t)di * L.T * DWR_ROWS + tile;
  unsigned* lat_stamp = DR.flags + 4 * L.T * DWR_ROWS + di * L.B + tile;
  const bool fault = DR.fault != 0 && bid == 0;
  if (DR.lat_split) {
    // the chain up to its last stage; the BPTT takes d h_T from the chain's gradient record in LDS (which lies behind everything the
    // BPTT keeps in LDS: seq_small_folddw_launch), and the chain's stores / atomics go out while the BPTT's weights travel
    latent_bwd_row_body<false>(LD, params, grads, tile, di, lds, 1);        // (ends behind a barrier)
    LSTAMP(4, 9);
    const float* dh_lds = lds + latent_bwd_grd_floats(LD.rec_size) + LD.in_off[di];
    MFM_TUPLE4(small_bwd_body_x<KQ, 1, 16, true, LatentDev>(d, L.T, L.B, tile, lds, stamp, epoch, fault, LD, params, grads, di, dh_lds, lat_stamp))
  } else {
    latent_bwd_row_body<false>(LD, params, grads, tile, di, lds);
    LSTAMP(4, 9);
    sync_stores();           // d h_T of this (row, encoder) is in memory (and the LDS is free) before the BPTT reads it
    LSTAMP(4, 8);
    if (threadIdx.x == 0) dwr_stamp(lat_stamp, epoch);
    MFM_TUPLE4(small_bwd_body<KQ, 1, 16, true>(d, L.T, L.B, tile, lds, stamp, epoch, fault))
  }
  LSTAMP_W(4, 15);
}

// Decoder recurrences with TAIL blocks (round 6): blocks [0, 3 B) are kernel4<false>'s rows of the three decoders; blocks
// [tail_begin, tail_begin + 4 B) finish the latent forward chains the encoder launch left behind the z -> f MLPs -- classifier,
// logvar heads, KLD and discriminative loss, y_hat, the rest of the saved record (latent_row_dev.h, mode 3).  Nothing in this
// launch waits for them; they run on CUs the 96 decoder rows leave idle.
template <int K0, int K1, int K2>
__global__ __launch_bounds__(1024) void lstm_seq_small_dectail_kernel(const SeqLaunch L, const LatentDev LD, const float* __restrict__ params,
                                                                      const int tail_begin) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int bid = blockIdx.x;
  LSTAMP(1, 0);
  if (bid >= tail_begin) {
    const int r = bid - tail_begin;
    latent_fwd_row_body<false>(LD, params, r % L.B, r / L.B, lds, true, 3);
    LSTAMP(1, 15);
    return;
  }
  MFM_SEQ_BLOCK_LSTM(L, bid, di)
  const SeqDev& d = L.d[di];
  const int tile = bid - d.block_begin;
  MFM_TUPLE3(small_fwd_body<KQ, 1>(d, L.T, L.B, tile, lds))
  LSTAMP(1, 15);
}

// Decoder BPTTs with HEAD blocks (round 6): blocks [0, 3 B) are kernel4<true>'s rows; blocks [head_begin, head_begin + 4 B) run the
// part of the latent BACKWARD chains that does not wait for the decoders (latent_row_dev.h, mode 3) on CUs the 96 rows leave idle.
template <int K0, int K1, int K2>
__global__ __launch_bounds__(1024) void lstm_seq_small_decbwd_head_kernel(const SeqLaunch L, const LatentDev LD, const float* __restrict__ params,
                                                                          float* __restrict__ grads, const int head_begin) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int bid = blockIdx.x;
  LSTAMP(3, 0);
  if (bid >= head_begin) {
    const int r = bid - head_begin;
    latent_bwd_row_body<false>(LD, params, grads, r % L.B, r / L.B, lds, 3);
    LSTAMP(3, 15);
    return;
  }
  MFM_SEQ_BLOCK_LSTM(L, bid, di)
  const SeqDev& d = L.d[di];
  const int tile = bid - d.block_begin;
  MFM_TUPLE3(small_bwd_body<KQ, 1, 16>(d, L.T, L.B, tile, lds))
  LSTAMP(3, 15);
}

// `no_panel` (forward, one-row tiles, every h % 4 == 0): the weights go straight into registers, the panel is not needed
static size_t small_lds_bytes(const SeqLaunch& L, bool bwd, int R, bool no_panel = false) {
  size_t lds_bytes = 0;
  for (int i = 0; i < L.count; ++i) {
    const SeqDev& d = L.d[i];
    const size_t HK = (size_t)d.hk4 * 4;
    const size_t HKB = (HK + 15) / 16 * 16;
    const size_t hh = no_panel ? 0 : (size_t)d.h * d.h;
    // forward: h ring + max(weight panel, output record + x-projection record); backward: dA ring +
    // saved-activation record + weight panel (see the bodies)
    const size_t rec = (2 * 6 + 2 * 4) * HKB * R;
    // backward, one-row tiles: the weight panel holds two gates (stage_gates2)
    const size_t need = (bwd ? (2 * 4 + 2 * 7) * HKB * R + (R == 1 ? 2 : 1) * hh : 2 * HKB * R + (2 * hh > rec ? 2 * hh : rec)) * sizeof(float);
    if (need > lds_bytes) lds_bytes = need;
  }
  return (lds_bytes + 15) / 16 * 16;
}

int seq_small_launch(SeqLaunch& L, bool bwd, hipStream_t stream) {
  LSTAMP_BIND();
  int max_threads = 64;
  for (int i = 0; i < L.count; ++i)
    if (8 * L.d[i].Hp > max_threads) max_threads = 8 * L.d[i].Hp;
  // Row-tile size.  Fewer rows per workgroup = shorter serial chain per time step (the step time is
  // VALU-issue bound: ~60 FMAs per thread and row), and that outweighs running several rounds of
  // workgroups per CU for as long as measured: 1-row tiles win up to 6 workgroups per CU (B=32..384 with four
  // LSTMs per launch: +12 % per step at B=128/256 over 2- and 4-row tiles), 4-row tiles from there on
  // (B=512: 0.856 vs 0.948 ms); 2-row tiles never did (profiles/r01l_rows_per_workgroup.txt).  Only the
  // pre-instantiated size tuples have R < 4 variants.
  int R = ((long)L.count * L.B < 6L * device_cus()) ? 1 : 4;
  if (const char* e = opt_get("MFM_SEQ_ROWS")) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4) R = v; }
  for (int attempt = 0; attempt < 2; ++attempt) {
    int total = lay_out_blocks(L, cdiv(L.B, R));
    const size_t lds_bytes = small_lds_bytes(L, bwd, R);
    int rc = MFM_OK;
    bool done = false;
    // forward, one-row tiles: a few more blocks write this step's transposed-weight images
    L.n_img_blocks = 0;
    if (!bwd && R == 1 && L.n_img > 0) total = add_img_writers(L, total);
    // backward, one-row tiles: MFM_SEQ_KS=8 selects 8 k-slices per unit pair (half the threads, twice the FMAs each).
    // Opt-in: measured equal (encoders 30.5 vs 29.8 us) or slower (decoders 37.9 vs 32.6 us, 24 spilled registers) at B=32
    // (profiles/r02_seq_ks8.txt) -- the step is a latency chain (LDS hand-over, barrier, reduction), not issue-bound enough
    // for fewer, fatter waves to pay
    bool fat = false;
    if (const char* e = opt_get("MFM_SEQ_KS")) fat = bwd && R == 1 && max_threads / 2 <= 512 && atoi(e) == 8;
    if (fat) done = try_all_fat(L, total, max_threads / 2, lds_bytes, stream, &rc);
    // bf16 plans, forward, one-row tiles: the decoders' recurrent product on v_dot2c_f32_bf16 (opt-in, small_fwd_body<.., BF>)
    if (!done && !bwd && R == 1 && L.bf16_dot && seq_is_tuple(L, kDecHk4, 3, -1)) {
      rc = seq_launch_kernel(lstm_seq_small_kernel4<false, 1, 16, 26, 6, 6, 0, 0, 0, true>, "lstm_seq_small_fwd_kernel4", dim3(total), dim3(max_threads),
                             lds_bytes, stream, nullptr, L);
      done = true;
    }
    if (!done) done = R == 1 ? try_all<1>(L, bwd, total, max_threads, lds_bytes, stream, &rc)
                    : R == 2 ? try_all<2>(L, bwd, total, max_threads, lds_bytes, stream, &rc)
                             : try_all<4>(L, bwd, total, max_threads, lds_bytes, stream, &rc);
    if (done) {
      if (rc == MFM_OK && L.n_img_blocks == 0) L.n_img = 0;        // (tells the caller that no images were written)
      return rc;
    }
    R = 4;    // no specialised kernel for this size tuple: generic 16-variant kernel, 4-row tiles
  }
  L.n_img = 0; L.n_img_blocks = 0;
  const int total = lay_out_blocks(L, cdiv(L.B, 4));
  return seq_launch_kernel(bwd ? lstm_seq_small_kernel<true> : lstm_seq_small_kernel<false>, bwd ? "lstm_seq_small_bwd_kernel" : "lstm_seq_small_fwd_kernel",
                           dim3(total), dim3(max_threads), small_lds_bytes(L, bwd, 4), stream, nullptr, L);
}

// The launchers below: MFM_OK: launched.  MFM_ERR_UNSUPPORTED: not a case the kernel takes (the caller issues the separate
// launches); each is its predicate plus the block layout.
// Whether the plan may use the role-workgroup launches at all is the plan's "handover" option (plan.hip): the in-launch
// hand-overs count on this launch becoming resident workgroup by workgroup in block order; launches of two queues that
// together exceed the CUs can block each other's producers until the waits give up (status word, poisoned gradient guard).
static bool fold_enabled() { return !opt_disabled("MFM_LATENT_FOLD") && !seq_tuning_overrides(); }

bool seq_small_folddw_supported(int T, int B) {
  if (opt_disabled("MFM_DW_FOLD") || !fold_enabled()) return false;
  return T >= 1 && B >= 1 && B <= DWR_ROWS && device_cus() - 4 * B >= 32;
}

int seq_small_folddw_launch(SeqLaunch& L, const LatentDev& LD, DwRole& DR, const float* params, float* grads, hipStream_t stream) {
  if (!seq_is_tuple(L, kEncHk4, 4, 0) || !chain_rows_match(LD, L.B) || !seq_small_folddw_supported(L.T, L.B)) return MFM_ERR_UNSUPPORTED;
  LSTAMP_BIND();
  const int n_role = DR.n_role;          // the block table was laid out for this many role workgroups
  if (n_role < 1 || n_role > device_cus() - 4 * L.B) return MFM_ERR_UNSUPPORTED;
  DR.T = L.T; DR.B = L.B;
  const int total = lay_out_blocks(L, L.B) + n_role;
  size_t lds_bytes = small_lds_bytes(L, true, 1);
  const size_t role = (size_t)DWR_LDS_FLOATS * sizeof(float);      // one shared A image + four B images + the pipeline's answer word + the block records
  if (DR.n_iter * 4 > DWR_MAXREC) return MFM_ERR_UNSUPPORTED;
  // the chain's gradient record must survive into the BPTT's prologue: it has to lie behind everything the BPTT keeps in LDS, and
  // every encoder must take its transposed weights from this step's images (no staging panel)
  DR.lat_split = 0;
  if (!opt_disabled("MFM_LATENT_SPLIT")) {
    bool imgs = true;
    for (int i = 0; i < 4; ++i) imgs = imgs && L.d[i].wt_img != nullptr;
    if (imgs && lds_bytes <= (size_t)latent_bwd_grd_floats(LD.rec_size) * sizeof(float)) DR.lat_split = 1;
  }
  lds_bytes = std::max(lds_bytes, std::max(chain_lds_bytes(LD, true), role));
  if (lds_bytes > 160 * 1024) return MFM_ERR_UNSUPPORTED;
  return seq_launch_kernel(lstm_seq_small_folddw_kernel<8, 2, 20, 30>, "lstm_seq_small_folddw_kernel", dim3(total), dim3(1024), lds_bytes, stream, nullptr,
                           L, LD, DR, params, grads);
}

// Can the decoder launch of this plan carry the tail blocks?  (asked by the encoder launch before it leaves the tails behind)
bool seq_small_dectail_supported(int T, int B, const int* dec_h, const LatentDev& LD) {
  if (opt_disabled("MFM_LATENT_TAIL") || seq_tuning_overrides() || opt_get("MFM_BF16_DOT")) return false;
  for (int i = 0; i < 3; ++i)
    if (round_up(cdiv(dec_h[i], 4), 2) != kDecHk4[i]) return false;
  if (!chain_rows_match(LD, B) || LD.tail_from < 1 || LD.tail_from >= LD.nstages) return false;
  return T >= 1 && 3 * B + 4 * B <= device_cus();
}
static bool dectail_takes(const SeqLaunch& L, const LatentDev& LD) {
  if (!seq_is_tuple(L, kDecHk4, 3, 1)) return false;
  const int hh[3] = {L.d[0].h, L.d[1].h, L.d[2].h};
  return seq_small_dectail_supported(L.T, L.B, hh, LD);
}

// decoder rows + tail blocks.  MFM_ERR_UNSUPPORTED: the caller runs the tails as a launch of their own.
int seq_small_dectail_launch(SeqLaunch& L, const LatentDev& LD, const float* params, hipStream_t stream) {
  LSTAMP_BIND();
  if (L.bf16_dot || !dectail_takes(L, LD)) return MFM_ERR_UNSUPPORTED;
  bool direct = true;
  for (int i = 0; i < 3; ++i) direct = direct && (L.d[i].h & 3) == 0 && L.d[i].wf_img && L.d[i].wf1_img;
  const int tail_begin = lay_out_blocks(L, L.B), total = tail_begin + 4 * L.B;
  L.n_img = 0; L.n_img_blocks = 0;
  const size_t lds_bytes = std::max(chain_lds_bytes(LD, false), small_lds_bytes(L, false, 1, direct));
  if (lds_bytes > 160 * 1024) return MFM_ERR_UNSUPPORTED;
  // (1024 threads: the chain's work items are tabulated for them)
  return seq_launch_kernel(lstm_seq_small_dectail_kernel<26, 6, 6>, "lstm_seq_small_dectail_kernel", dim3(total), dim3(1024), lds_bytes, stream, nullptr,
                           L, LD, params, tail_begin);
}

// decoder BPTT rows + head blocks.  MFM_ERR_UNSUPPORTED: the caller runs the plain BPTT launch, the encoder launch its whole chain.
int seq_small_decbwd_head_launch(SeqLaunch& L, const LatentDev& LD, const float* params, float* grads, hipStream_t stream) {
  LSTAMP_BIND();
  if (opt_disabled("MFM_LATENT_BWD_HEAD") || !dectail_takes(L, LD) || !LD.grd_out) return MFM_ERR_UNSUPPORTED;
  for (int i = 0; i < 3; ++i)
    if (!L.d[i].wt_img) return MFM_ERR_UNSUPPORTED;
  const int head_begin = lay_out_blocks(L, L.B), total = head_begin + 4 * L.B;
  const size_t lds_bytes = std::max(chain_lds_bytes(LD, true), small_lds_bytes(L, true, 1));
  if (lds_bytes > 160 * 1024) return MFM_ERR_UNSUPPORTED;
  return seq_launch_kernel(lstm_seq_small_decbwd_head_kernel<26, 6, 6>, "lstm_seq_small_decbwd_head_kernel", dim3(total), dim3(1024), lds_bytes, stream,
                           nullptr, L, LD, params, grads, head_begin);
}

// Projection role workgroups for a forward fold launch: shapes the role kernel takes and enough idle CUs
bool seq_small_foldproj_supported(int T, int B, const int* h, const int* k, int n_enc) {
  if (opt_disabled("MFM_PROJ_FOLD") || !fold_enabled()) return false;
  if (n_enc != 4 || T < 1 || B < 1 || B > PROJ_ROLE_CB) return false;
  if (device_cus() - 4 * B < PROJ_ROLE_SLOTS) return false;
  int slots = 0, kmax = 0;
  for (int e = 0; e < 4; ++e) {
    if (k[e] < 1 || k[e] > 128 * PROJ_ROLE_MAXG) return false;
    slots += 4 * round_up(h[e], 16) / PROJ_ROLE_CB;
    if (4 * round_up(h[e], 16) / PROJ_ROLE_CB > PROJ_ROLE_FLAGS) return false;
    kmax = std::max(kmax, k[e]);
  }
  if (slots > PROJ_ROLE_SLOTS) return false;
  const int ks = proj_role_kstride(kmax);
  return ((size_t)2 * PROJ_ROLE_CB * ks + 16 * PROJ_ROLE_PW) * sizeof(float) <= 160 * 1024;
}

int seq_small_foldproj_launch(SeqLaunch& L, const LatentDev& LD, ProjRole& PR, const float* params, hipStream_t stream) {
  if (!seq_is_tuple(L, kEncHk4, 4, 0) || !chain_rows_match(LD, L.B)) return MFM_ERR_UNSUPPORTED;
  int hh[4], kk[4];
  for (int i = 0; i < 4; ++i) { hh[i] = L.d[i].h; kk[i] = PR.e[i].k; }
  if (!seq_small_foldproj_supported(L.T, L.B, hh, kk, 4)) return MFM_ERR_UNSUPPORTED;
  LSTAMP_BIND();
  int n_role = (device_cus() - 4 * L.B) / PROJ_ROLE_SLOTS * PROJ_ROLE_SLOTS;
  if (const char* e = opt_get("MFM_PROJ_FOLD_ROLES")) { const int v = atoi(e) / PROJ_ROLE_SLOTS * PROJ_ROLE_SLOTS; if (v >= PROJ_ROLE_SLOTS) n_role = v; }
  PR.n_role = n_role; PR.groups = n_role / PROJ_ROLE_SLOTS;
  if (!PR.words || ((uintptr_t)PR.words & 7) != 0) return MFM_ERR_UNSUPPORTED;      // (64-bit atomics: naturally aligned words)
  int kmax = 0, cb = 0;
  PR.w_ld = 0;
  for (int i = 0; i < 4; ++i) {
    kmax = std::max(kmax, PR.e[i].k);
    PR.e[i].cb_begin = cb; PR.e[i].ncb = 4 * L.d[i].Hp / PROJ_ROLE_CB;
    cb += PR.e[i].ncb;
    PR.e[i].w_off = PR.w_ld; PR.w_ld += 4 * L.d[i].Hp;       // a row of words: the encoders' 4 Hp gate columns side by side
  }
  PR.kstride = proj_role_kstride(kmax);
  const int total = lay_out_blocks(L, L.B, n_role);
  const size_t role = ((size_t)2 * PROJ_ROLE_CB * PR.kstride + 16 * PROJ_ROLE_PW) * sizeof(float);
  size_t lds_bytes = std::max(small_lds_bytes(L, false, 1), std::max(chain_lds_bytes(LD, false), role));
  // chain tables preloaded in front of the time loop: chain region + recurrence buffers side by side (lstm_seq_small_foldproj_kernel)
  PR.lat_pre = 0;
  if (!opt_disabled("MFM_LATENT_PRELOAD")) {
    bool direct = true;
    for (int i = 0; i < 4; ++i) direct = direct && (L.d[i].h & 3) == 0;
    const size_t side = chain_lds_bytes(LD, false) + small_lds_bytes(L, false, 1, true);
    if (direct && side <= 160 * 1024) { PR.lat_pre = 1; lds_bytes = std::max(side, role); }
  }
  if (!PR.lat_pre) PR.lat_tail = 0;          // (the head / tail split is a form of the preloaded chain)
  if (lds_bytes > 160 * 1024) return MFM_ERR_UNSUPPORTED;
  return seq_launch_kernel(lstm_seq_small_foldproj_kernel<8, 2, 20, 30>, "lstm_seq_small_foldproj_kernel", dim3(total), dim3(1024), lds_bytes, stream, nullptr,
                           L, LD, PR, params);
}

int seq_small_fold_launch(SeqLaunch& L, bool bwd, const LatentDev& LD, const float* params, float* grads, hipStream_t stream) {
  if (!fold_enabled() || !seq_is_tuple(L, kEncHk4, 4, 0) || !chain_rows_match(LD, L.B)) return MFM_ERR_UNSUPPORTED;
  if (!((long)L.count * L.B < 6L * device_cus())) return MFM_ERR_UNSUPPORTED;          // one-row tiles only
  int max_threads = 1024;       // the chain's work items are tabulated for up to 1024 threads
  for (int i = 0; i < 4; ++i)
    if (8 * L.d[i].Hp > max_threads) max_threads = 8 * L.d[i].Hp;
  int total = lay_out_blocks(L, L.B);
  L.n_img_blocks = 0;
  if (!bwd && L.n_img > 0) total = add_img_writers(L, total);
  const size_t lds_bytes = std::max(small_lds_bytes(L, bwd, 1), chain_lds_bytes(LD, bwd));
  if (lds_bytes > 160 * 1024) return MFM_ERR_UNSUPPORTED;
  return seq_launch_kernel(bwd ? lstm_seq_small_fold_kernel<true, 8, 2, 20, 30> : lstm_seq_small_fold_kernel<false, 8, 2, 20, 30>, "lstm_seq_small_fold_kernel",
                           dim3(total), dim3(max_threads), lds_bytes, stream, nullptr, L, LD, params, grads);
}

}  // namespace mfm
