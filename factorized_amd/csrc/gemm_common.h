// Shared between the fp32 (gemm.hip) and bf16-operand (gemm_bf16.hip) grouped GEMM kernels and, as far as it applies, the
// small-row weight-gradient kernel (gemm_tn.hip): the problem table that travels in the kernel-argument segment, the rules
// that host and kernels must state alike (an operand's form and extent, which workgroup computes which tile) and the
// common epilogue (bias, alpha, pad columns, atomics for split-K / accumulating problems, squared-error epilogue,
// zero-fill spans).
#pragma once
#include "internal.h"

namespace mfm {

// ---------------------------------------------------------------- operand form and extent: one statement for host and kernels
// How an operand lies in memory, seen from a thread's 4-element load group: unit-stride along k (x, h, W of a forward
// product), unit-stride along its rows (m for a, n for b: both operands of a weight-gradient product), or neither.  The
// first two are fetched 16 bytes at a time; one odd operand puts its whole group on the dword loads of the fp32 kernel.
enum GemmForm { GEMM_K_CONTIG, GEMM_ROW_CONTIG, GEMM_ODD };
__host__ __device__ inline GemmForm gemm_operand_form(const int64_t s_row, const int64_t s_k) {
  return (s_k == 1) ? GEMM_K_CONTIG : (s_row == 1 ? GEMM_ROW_CONTIG : GEMM_ODD);
}

// Elements from the first to the last element of one batch member of a rows x cols operand, and the same in bytes: the
// extent of the kernels' bounds-checked buffer descriptors, which end at the last addressable element (a 16-byte group
// that runs past it reads zeros).  An empty axis counts as one element.  2-byte elements (bf16-resident operands) are
// rounded up to whole dwords: the range check is per dword, an odd element count would zero the last element.  The kernels
// instantiate it with the 32-bit ints of their offsets, the host with int64_t to refuse what those cannot hold.
template <typename I>
__host__ __device__ inline I gemm_operand_elems(const I rows, const I cols, const I s_row, const I s_col) {
  return ((rows > 1 ? rows : 1) - 1) * s_row + ((cols > 1 ? cols : 1) - 1) * s_col + 1;
}
template <typename I>
__host__ __device__ inline I gemm_operand_bytes(const I rows, const I cols, const I s_row, const I s_col, const int elem_bytes) {
  const I e = gemm_operand_elems(rows, cols, s_row, s_col);
  return (elem_bytes == 2) ? ((e * 2 + 3) & ~(I)3) : e * 4;
}

#define MFM_GEMM_NEPI 4     // problems per launch that may carry an output transform (always the first ones)

struct GemmProblem {
  MfmGemmDesc d;
  int tiles_m, tiles_n, block_begin, k_per_split;
};
struct GemmGroup {
  GemmProblem p[MFM_GEMM_MAXP];
  int begins[MFM_GEMM_MAXP];     // first workgroup of every problem (INT_MAX past `count`): found with one unrolled compare chain
  int count;
  // optional: spans the launch also clears (the fused step's loss slots and gradient buffer ride on its
  // first GEMM instead of two memset launches of ~4.7 us each)
  float* zero_ptr[MFM_GEMM_ZSPANS];
  int64_t zero_n[MFM_GEMM_ZSPANS];
  // optional: squared-error epilogue for the first mse_count problems (decoder fc1 -> x_hat): the tile that
  // produced x_hat also forms d x_hat and its share of the reconstruction loss (mfm_mosi.py:441-446), so the
  // separate elementwise launch and its re-read of x_hat disappear
  MseEpi mse[3];
  int mse_count;
  // optional: per-problem output transforms (internal.h::GemmEpi), first epi_count problems
  GemmEpi epi[MFM_GEMM_NEPI];
  int epi_count, epi_train;
  unsigned long long epi_seed;
  const unsigned long long* epi_tick;
};
__host__ __device__ inline int gemm_problem_batch(const GemmProblem& P) { return P.d.batch; }
__host__ __device__ inline int gemm_problem_k(const GemmProblem& P) { return P.d.k; }

// Host: begins[i] holds the workgroup count of problem i on entry and its first workgroup on return, as does
// p[i].block_begin; the entries past `count` are INT_MAX, which no workgroup id reaches.  Returns the grid size.
template <typename Group>
static inline int gemm_assign_blocks(Group& g) {
  constexpr int MAXP = sizeof(g.begins) / sizeof(g.begins[0]);
  int total = 0;
  for (int i = 0; i < g.count; ++i) {
    const int blocks = g.begins[i];
    g.p[i].block_begin = g.begins[i] = total;
    total += blocks;
  }
  for (int i = g.count; i < MAXP; ++i) g.begins[i] = 0x7fffffff;
  return total;
}

// Which tile of which problem a workgroup computes (wave-uniform).  Group is a problem table with p[], begins[] and
// count whose problems carry tiles_m, tiles_n, block_begin, k_per_split and answer gemm_problem_batch / gemm_problem_k.
// The logical order inside a problem is (split, z, tm, tn), tn fastest; kbeg >= kend marks a K range with nothing in it.
struct GemmTile { int pi, tm, tn, z, split, m0, n0, kbeg, kend; };
template <typename Group>
__device__ __forceinline__ GemmTile gemm_locate(const Group& g, const int BM, const int BN) {
  constexpr int MAXP = sizeof(g.begins) / sizeof(g.begins[0]);
  GemmTile t;
  t.pi = 0;
  const int bid = blockIdx.x;
#pragma unroll
  for (int i = 1; i < MAXP; ++i) t.pi += (bid >= g.begins[i]) ? 1 : 0;
  const auto& P = g.p[t.pi];
  int local = bid - P.block_begin;
  {
    // Workgroups are dealt to the 8 XCDs round-robin by id, and each XCD has its own L2.  Tiles that share
    // an operand panel (same m-tile across n, same n-tile across m / gates) are neighbours in the LOGICAL
    // order, so inside every problem each XCD is given one contiguous run of logical tiles: a panel is then
    // fetched from HBM once per XCD that needs it instead of once per tile (the LSTM weight-gradient launch
    // read 37.7 MB for ~6 MB of operands before this, the small-row one 45 MB for ~8 MB), while every XCD still
    // gets an equal share of every problem (a whole-launch remap left the XCDs with the long-K problems as stragglers).
    constexpr int NX = 8;
    const int nb = ((t.pi + 1 < g.count) ? g.begins[t.pi + 1] : (int)gridDim.x) - P.block_begin;
    const int x = local % NX, j = local / NX;
    const int per = nb / NX, rem = nb % NX;
    local = x * per + (x < rem ? x : rem) + j;
  }
  const int batch = gemm_problem_batch(P);
  t.tn = local % P.tiles_n; local /= P.tiles_n;
  t.tm = local % P.tiles_m; local /= P.tiles_m;
  t.z = local % batch;
  t.split = local / batch;
  t.m0 = t.tm * BM; t.n0 = t.tn * BN;
  t.kbeg = t.split * P.k_per_split;
  t.kend = min(gemm_problem_k(P), t.kbeg + P.k_per_split);
  return t;
}

// The squared-error targets of this thread's outputs (clamped into x: the epilogue uses only those inside), requested
// ahead of the K loop; and the accumulator clear.
template <int FR, int TF>
__device__ __forceinline__ void gemm_mse_targets(const MseEpi& me, const bool do_mse, const MfmGemmDesc& d, const GemmTile& t,
                                                 const int wm, const int wn, const int bi, const int q, float (&tgt)[TF][TF][4]) {
  if constexpr (FR <= 2) if (do_mse) {
#pragma unroll
    for (int fm = 0; fm < FR; ++fm)
#pragma unroll
      for (int fn = 0; fn < FR; ++fn)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = min(t.m0 + wm * 16 * FR + fm * 16 + q * 4 + r, d.m - 1);
          const int col = min(t.n0 + wn * 16 * FR + fn * 16 + bi, max(d.n_valid - 1, 0));
          tgt[fm][fn][r] = me.x[(int64_t)row * me.ldx + col];
        }
  }
}
template <int FR>
__device__ __forceinline__ void gemm_clear_acc(f32x4 (&acc)[FR][FR]) {
#pragma unroll
  for (int i = 0; i < FR; ++i)
#pragma unroll
    for (int j = 0; j < FR; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// Epilogue of one workgroup tile.  acc[fm][fn] follows the 16x16 MFMA accumulator map (row = 4*(lane>>4) + r,
// col = lane & 15), identical for the f32 and bf16 instructions.
template <int FR, int TF>
__device__ __forceinline__ void gemm_epilogue(const GemmGroup& g, const MfmGemmDesc& d, const GemmTile& t, const int wm, const int wn,
                                              const int bi, const int q, const int tid, const int lane, const int wave,
                                              f32x4 (&acc)[FR][FR], float (&tgt)[TF][TF][4], const bool do_mse) {
  const int pi = t.pi, z = t.z, split = t.split, m0 = t.m0, n0 = t.n0;
  const MseEpi& me = g.mse[do_mse ? pi : 0];
  float* __restrict__ C = d.c ? d.c + (int64_t)z * d.c_sz : nullptr;
  float* __restrict__ C2 = d.c2 ? d.c2 + (int64_t)z * d.c_sz : nullptr;
  // c_bf16 (bf16-resident outputs of a bf16 plan: the x-projection, dH): the same element offsets, 2-byte elements
  const bool c16 = d.c_bf16 != 0;
  __bf16* __restrict__ C16 = reinterpret_cast<__bf16*>(d.c) + (int64_t)z * d.c_sz;
  __bf16* __restrict__ C216 = reinterpret_cast<__bf16*>(d.c2) + (int64_t)z * d.c_sz;
  float sq = 0.0f;
#pragma unroll
  for (int fm = 0; fm < FR; ++fm)
#pragma unroll
    for (int fn = 0; fn < FR; ++fn) {
      const int col = n0 + wn * 16 * FR + fn * 16 + bi;
      if (col >= d.n) continue;
      float bsum = 0.0f;
      if (split == 0 && col < d.n_valid) {
        if (d.bias) bsum += d.bias[(int64_t)z * d.bias_sz + col];
        if (d.bias2) bsum += d.bias2[(int64_t)z * d.bias_sz + col];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm * 16 * FR + fm * 16 + q * 4 + r;
        if (row >= d.m) continue;
        float v = (col < d.n_valid) ? d.alpha * acc[fm][fn][r] + bsum : 0.0f;
        const int64_t off = (int64_t)row * d.ldc + col;
        if (pi < g.epi_count && col < d.n_valid) {          // wave-uniform condition on pi
          const GemmEpi& ep = g.epi[pi];
          if (ep.kind == 1) {
            float mk = 1.0f;
            if (g.epi_train && ep.p > 0.0f) {
              const uint64_t idx = ((uint64_t)ep.op_id << 40) + (uint64_t)row * (uint64_t)d.n_valid + (uint64_t)col;
              mk = (rng_uniform(g.epi_seed + (g.epi_tick ? *g.epi_tick : 0ull), idx) < ep.p) ? 0.0f : 1.0f / (1.0f - ep.p);
            }
            ep.aux[off] = (v > 0.0f) ? mk : 0.0f;
            v = fmaxf(v, 0.0f) * mk;
          } else if (ep.kind == 2) {
            v = act_tanh(v);
          } else if (ep.kind == 3) {
            v *= ep.aux[off];
          }
        }
        if (d.accumulate) {
          if (col < d.n_valid) {
            atomicAdd(C + off, v);
            if (C2) atomicAdd(C2 + off, v);
          }
        } else {
          if (c16) {
            C16[off] = (__bf16)v;
            if (C2) C216[off] = (__bf16)v;
          } else {
            if (C) C[off] = v;          // (null: a training step needs the squared error and d x_hat only, not x_hat itself)
            if (C2) C2[off] = v;
          }
          if (do_mse && col < d.n_valid) {
            const float diff = v - tgt[fm % TF][fn % TF][r];
            sq += diff * diff;
            if (me.dxhat) {
              const int64_t doff = me.ld_dxhat ? (int64_t)row * me.ld_dxhat + col : off;
              if (me.dxhat_bf16) reinterpret_cast<__bf16*>(me.dxhat)[doff] = (__bf16)(me.grad_scale * diff);
              else me.dxhat[doff] = me.grad_scale * diff;
            }
          }
        }
      }
    }
  if (do_mse && me.loss) {
    __shared__ float sqsum[4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
    if (lane == 0) sqsum[wave] = sq;
    lds_barrier();
    if (tid == 0) atomicAdd(me.loss, (sqsum[0] + sqsum[1] + sqsum[2] + sqsum[3]) * me.inv_count);
  }
  // zero-fill spans last: ahead of the K loop these stores would sit in front of the first tile loads in the
  // in-order vmcnt queue and put a store round trip on every workgroup's critical path
#pragma unroll
  for (int zi = 0; zi < MFM_GEMM_ZSPANS; ++zi) {
    if (g.zero_n[zi] > 0) {          // 16-byte aligned, multiple of 4 floats (checked by the host)
      f32x4* z4 = reinterpret_cast<f32x4*>(g.zero_ptr[zi]);
      const int64_t n4 = g.zero_n[zi] >> 2;
      for (int64_t i = (int64_t)blockIdx.x * 256 + tid; i < n4; i += (int64_t)gridDim.x * 256) z4[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
}

// gemm_bf16.hip: the bf16-operand kernel with 32 FR x 32 FR tiles (FR = 1, 2, 4)
typedef void (*GemmKernel)(const GemmGroup);
GemmKernel gemm_bf16_kernel_for(int FR);
constexpr int BKB = 64;   // K depth of one LDS stage of the bf16 kernel: two 32-deep MFMA k-steps

}  // namespace mfm
