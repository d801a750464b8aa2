// The decoders' recurrence of the ablation entries (ablation.hip: M_B; ablation_mfn.hip: M_A, M_C): decode_plain_kernel
// (missing.hip) behind its two dense layers -- the embedding of a row is read where an earlier launch of the call left it, a column
// range of the chunk's embedding block in the workspace, and h_t alone is stored, for fc1_sqerr_kernel behind the launch.
#pragma once
#include "infer_dev.h"

namespace mfm {

#define ABL_MODS 3

struct AblDec {
  SeqDev seq;                                  // w_ih, w_hh, b_ih, b_hh, h = the embedding's width, Hp, hk4, is_dec; hs: this chunk's [T, n, Hp]
  int col, block_begin;                        // the first column of the embedding in a row of the block
};
struct AblDecDev { AblDec d[ABL_MODS]; const float* f; int count, T, n, ftot, seq_floats; };      // f: the block [n, ftot]

// SAME: the three decoders have one hidden size (those of M_A and M_C, which read the same embedding): every block runs the body
// of K0 whatever its decoder, so one launch covers any size without a per-block switch
template <int R, int K0, int K1, int K2, bool SAME = false>
__global__ __launch_bounds__(1024) void ablation_decode_kernel(const AblDecDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, bid = blockIdx.x;
  MFM_SEQ_BLOCK_LSTM(P, bid, di)
  const AblDec& D = P.d[di];
  const int tile = bid - D.block_begin, b0 = tile * R;
  const int h = D.seq.h;
  // behind everything the recurrence uses: the embedding must survive its weight staging.  [R][h]: the recurrence's h_init
  float* emb = lds + P.seq_floats;
  for (int e = tid; e < h * R; e += blockDim.x) {
    const int r = e / h, k = e - r * h;
    emb[e] = (b0 + r < P.n) ? P.f[(int64_t)(b0 + r) * P.ftot + D.col + k] : 0.0f;
  }
  lds_barrier();
  // the tile as a batch of its own: row r of the embedding in LDS is row r of the recurrence, and of this tile's part of hs
  SeqDev d = D.seq;
  d.h_init = emb; d.ld_init = h;
  d.hs = D.seq.hs + (int64_t)b0 * D.seq.Hp;
  const int rows = min(R, P.n - b0);
  const int64_t hs_step = (int64_t)P.n * D.seq.Hp;
  if constexpr (SAME) {
    small_fwd_body<K0, R, false, false, false, true>(d, P.T, rows, 0, lds, nullptr, 0u, 0, HoCtl{nullptr, nullptr, nullptr, 5000000ll, 1u}, hs_step);
  } else {
    MFM_TUPLE3((small_fwd_body<KQ, R, false, false, false, true>(d, P.T, rows, 0, lds, nullptr, 0u, 0,
                                                                  HoCtl{nullptr, nullptr, nullptr, 5000000ll, 1u}, hs_step)))
  }
}

// the launch(es) of a chunk of P.n rows in tiles of R rows: `canon` names the hk4 tuple the per-block switch is instantiated for
// (the launch rules of infer_dev.h)
template <int R, int C0, int C1, int C2>
static int abl_decode_launch(const char* who, AblDecDev& P, int threads, size_t lds_bytes, hipStream_t stream) {
  const bool canon = P.d[0].seq.hk4 == C0 && P.d[1].seq.hk4 == C1 && P.d[2].seq.hk4 == C2;
  return infer_launch_tuple_or_each<R>(who, "ablation_decode_kernel", P, canon ? ablation_decode_kernel<R, C0, C1, C2> : nullptr,
                                       [](auto kk) { return ablation_decode_kernel<R, decltype(kk)::value, 0, 0>; }, threads, lds_bytes, stream);
}

// three decoders of ONE hidden size: one launch of 3 x tiles workgroups of the kernel instantiated for that size alone
template <int R>
static int abl_decode_launch_same(const char* who, AblDecDev& P, size_t lds_bytes, hipStream_t stream) {
  const int tiles = cdiv(P.n, R);
  for (int i = 0; i < ABL_MODS; ++i) P.d[i].block_begin = i * tiles;
  return infer_launch_hk4(who, "ablation_decode_kernel", P.d[0].seq, [](auto kk) { return ablation_decode_kernel<R, decltype(kk)::value, 0, 0, true>; },
                          P, ABL_MODS * tiles, std::max(8 * P.d[0].seq.Hp, 64), lds_bytes, stream);
}

}  // namespace mfm
