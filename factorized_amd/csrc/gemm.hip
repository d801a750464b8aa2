// Grouped, batched, strided fp32 GEMM on v_mfma_f32_16x16x4_f32 (gfx950).
//
// One launch covers up to MFM_GEMM_MAXP independent problems (input projections of the 4
// encoders; all 49 weight-gradient products of the backward; ...), because at the MOSI batch
// size every one of them is far too small to fill 256 CUs on its own and a launch boundary costs
// several us (a grouped launch of this kernel has a ~7 us floor, profiles/r01 GEMM microbenchmark).  Tiles are 32x32 or 64x64 (picked so the group yields >= ~2 blocks
// per CU), K is staged 32 deep through LDS.  The LDS image follows the operand's memory order so that
// a thread's 4-element group is ONE ds_write_b128: [k][m+16] for m-/n-contiguous operands (MFMA
// operand reads conflict-free: row stride == 16 mod 32 banks), [m][k+4] for k-contiguous ones (reads
// at most 2-way).  Writing k-contiguous groups into a [k][m] image cost 8-way-conflicted ds_write_b32.
#include <stdlib.h>

#include "internal.h"
#include "gemm_common.h"

namespace mfm {

constexpr int BK = 32;   // K depth of one LDS stage: 8 MFMA k-steps between barriers

// VEC: every operand of every problem in the group is unit-stride along its 4-element load groups
// (true for all products of the MFM step); the 16-byte path is then unconditional.  A launch with
// an oddly strided operand uses the VEC=false instantiation (dword buffer loads) for the whole group: the m-/n-
// and k-contiguous operands of such a group keep their LDS images and masks, and every dword is clamped into the operand.
// Occupancy target (second launch-bounds argument = waves per SIMD): a K step is a chain of latencies (LDS
// write -> barrier -> fragment reads -> 8 MFMAs), so resident waves are what keeps the MFMA pipe fed.  The compiler
// reports 89 registers (VEC; 94 without) / 5 workgroups per CU for the 32x32 tiles and 157 (160) / 3 for the 64x64
// tiles, all four without scratch (profiles/gemm_family_refactor.txt); measured against the compiler's default (108 / 4
// and 188 / 2): +4 % on the whole step at B=2048, +1 % at B=32; 6 waves (80 registers, 4 spilled) gains nothing more.
// FR = 4: 128x128 tiles (each wave 64x64 = 16 accumulators) for launches with thousands of 64x64 tiles: twice the MFMA
// work per staged byte and per barrier of the FR = 2 variant; 2 workgroups per CU (73 KB of LDS).  Both FR = 4 forms
// spill: about 220 registers and 272 bytes of scratch per lane are reported for them, and 256 registers with 304 bytes
// for the bf16-operand kernel's FR = 4 form.
// It carries no squared-error epilogue (64 more live registers): launches that need one stay on FR <= 2.
template <int FR, bool VEC>
__global__ __launch_bounds__(256, (FR == 1) ? (VEC ? 5 : 4) : (FR == 2 ? 3 : 2)) void gemm_f32_kernel(const GemmGroup g) {
  constexpr int BT = 32 * FR;                     // tile edge, m and n alike
  constexpr int LDR = BT + 16;                    // [k][row] layout (m-/n-contiguous operands)
  constexpr int LDK = BK + 4;                     // [row][k] layout (k-contiguous operands)
  constexpr int EPT = BT * BK / 256;              // elements per thread and operand tile
  constexpr int SZ = (BK * LDR > BT * LDK) ? BK * LDR : BT * LDK;
  // two LDS images per operand: while the MFMAs of K-tile kt read image kt&1, the registers of tile kt+1 are
  // written to the other one, so a K step costs ONE barrier instead of two
  __shared__ __attribute__((aligned(16))) float As2[2][SZ];
  __shared__ __attribute__((aligned(16))) float Bs2[2][SZ];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int bi = lane & 15, q = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;

  const GemmTile t = gemm_locate(g, BT, BT);
  const MfmGemmDesc& d = g.p[t.pi].d;
  const int kbeg = t.kbeg, kend = t.kend;
  if (kbeg >= kend && t.split > 0) return;

  // Register ring of DEPTH K-tiles in flight.  At these sizes (K = 300..640, 8 MFMAs per wave and
  // tile) one workgroup's K loop is a chain of latencies and, above all, of vector-memory instructions:
  // measured ~10 B/clk/CU with dword loads whatever else was tuned.  So:
  //   (a) tiles are fetched with BUFFER loads, 16 bytes per lane wherever the operand is unit-stride
  //       along the thread's 4-element group (buffer_load_dwordx4 needs only 4-byte alignment); the
  //       descriptor's num_records makes reads past the end of the operand return 0, so a group may
  //       straddle a row end or the K tail without any branch -- invalid elements are zeroed by a
  //       MULTIPLY (a select/branch makes hipcc wait vmcnt(0) right behind the load);
  //   (b) the barriers are LDS-only (lds_barrier): __syncthreads() drains the ring with vmcnt(0);
  //   (c) the operand fragments of a tile are read from LDS before the first MFMA.
  constexpr int DEPTH = (FR == 1) ? 3 : (FR == 2 ? 2 : 1);
  constexpr int G = EPT / 4;
  float ra[DEPTH][EPT], rb[DEPTH][EPT];
  const int klast = max(kend - 1, 0);

  // One operand as this thread sees it: a for its rows m, b for its "rows" n.
  struct Operand {
    __amdgpu_buffer_rsrc_t res;
    bool rowcontig;                       // unit-stride along the rows: the 4-element groups and the LDS image run along them
    int rlim, s_row, s_k;                 // rows that exist (m / n_valid), element strides
    int l_row, l_k;                       // LDS strides of the image (block-uniform values, no divergent control flow)
    int gk[G], gr[G], base[G], st[G];     // loop-invariant, per group: k in the tile, row, offset of the clamped row, place in the image
  };
  // the extent in bytes for the bounds-checked descriptor and every `off * 4` below are 32-bit ints: the host refuses
  // operands whose span in BYTES does not fit one (gemm_check_problem)
  auto operand = [&](const float* p, const int bytes, const GemmForm form, const int r0, const int rlim, const int s_row, const int s_k) {
    Operand o;
    o.res = __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, bytes, 0x00020000);
    o.rowcontig = form == GEMM_ROW_CONTIG;
    o.rlim = rlim; o.s_row = s_row; o.s_k = s_k;
    o.l_row = o.rowcontig ? 1 : LDK; o.l_k = o.rowcontig ? LDR : 1;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int idx = (tid * G + g) * 4;
      const int k = o.rowcontig ? idx / BT : idx % BK;
      const int r = o.rowcontig ? idx % BT : idx / BK;
      o.gk[g] = k; o.gr[g] = r0 + r;
      o.base[g] = min(r0 + r, max(rlim - 1, 0)) * s_row;
      o.st[g] = r * o.l_row + k * o.l_k;
    }
    return o;
  };
  const int a_sm = (int)d.a_sm, a_sk = (int)d.a_sk, b_sk = (int)d.b_sk, b_sn = (int)d.b_sn;
  const Operand oa = operand(d.a + (int64_t)t.z * d.a_sz, gemm_operand_bytes(d.m, d.k, a_sm, a_sk, 4),
                             gemm_operand_form(d.a_sm, d.a_sk), t.m0, d.m, a_sm, a_sk);
  const Operand ob = operand(d.b + (int64_t)t.z * d.b_sz, gemm_operand_bytes(d.k, d.n_valid, b_sk, b_sn, 4),
                             gemm_operand_form(d.b_sn, d.b_sk), t.n0, d.n_valid, b_sn, b_sk);
  auto load_op = [&](float (&r)[EPT], const Operand& o, const int k0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const int gk = k0 + o.gk[g], gr = o.gr[g];
      f32x4 v;
      if constexpr (VEC) {
        const int off = o.base[g] + min(gk, klast) * o.s_k;
        v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(o.res, off * 4, 0, 0));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {       // the group runs along the rows for a row-contiguous operand (as the mask and st have it), along k otherwise
          const int off = o.rowcontig ? min(gr + e, max(o.rlim - 1, 0)) * o.s_row + min(gk, klast) * o.s_k
                                      : o.base[g] + min(gk + e, klast) * o.s_k;
          v[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(o.res, off * 4, 0, 0));
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int er = o.rowcontig ? gr + e : gr, ek = o.rowcontig ? gk : gk + e;
        r[4 * g + e] = v[e] * (float)((int)(er < o.rlim) & (int)(ek < kend));
      }
    }
  };
  auto store_op = [&](const float (&r)[EPT], const Operand& o, float* img) {
#pragma unroll
    for (int g = 0; g < G; ++g)
      *reinterpret_cast<f32x4*>(img + o.st[g]) = f32x4{r[4 * g], r[4 * g + 1], r[4 * g + 2], r[4 * g + 3]};
  };
  auto load_tiles = [&](int slot, int k0) { load_op(ra[slot], oa, k0); load_op(rb[slot], ob, k0); };
  auto store_tiles = [&](int slot, int img) { store_op(ra[slot], oa, As2[img]); store_op(rb[slot], ob, Bs2[img]); };

  // squared-error epilogue: the targets of this thread's outputs are requested before the K loop
  const bool do_mse = (FR <= 2) && t.pi < g.mse_count;          // wave-uniform
  constexpr int TF = (FR <= 2) ? FR : 1;            // FR = 4 has no squared-error epilogue: no target registers
  float tgt[TF][TF][4];
  gemm_mse_targets<FR, TF>(g.mse[do_mse ? t.pi : 0], do_mse, d, t, wm, wn, bi, q, tgt);
  f32x4 acc[FR][FR];
  gemm_clear_acc<FR>(acc);

  const int nkt = (kend - kbeg + BK - 1) / BK;
  // the ring is always filled DEPTH deep (tiles past the end load clamped addresses and are masked
  // to zero): no branch around a load anywhere
#pragma unroll
  for (int s = 0; s < DEPTH; ++s) load_tiles(s, kbeg + s * BK);
  store_tiles(0, 0);
  load_tiles(0, kbeg + DEPTH * BK);
  lds_barrier();
  // ring slot of K-tile kt is kt % DEPTH; slot 0 was just refilled with tile DEPTH
  for (int kt0 = 0; kt0 < nkt; kt0 += DEPTH) {
#pragma unroll
    for (int s = 0; s < DEPTH; ++s) {
      const int kt = kt0 + s;
      const int img = kt & 1;
      const float* As = As2[img];
      const float* Bs = Bs2[img];
      // operand fragments are read from LDS ahead of the MFMAs that use them: the whole tile for the 32x32
      // variant, half a tile at a time for the 64x64 one (its 4 accumulators already fill the register budget
      // that decides between 2 and 3 waves per SIMD)
      constexpr int KSB = (FR == 1) ? BK / 4 : (FR == 2 ? BK / 8 : BK / 16);
#pragma unroll
      for (int kb = 0; kb < BK / 4; kb += KSB) {
        float af[KSB][FR], bf[KSB][FR];
#pragma unroll
        for (int ks = 0; ks < KSB; ++ks)
#pragma unroll
          for (int f = 0; f < FR; ++f) {
            af[ks][f] = As[((kb + ks) * 4 + q) * oa.l_k + (wm * 16 * FR + f * 16 + bi) * oa.l_row];
            bf[ks][f] = Bs[((kb + ks) * 4 + q) * ob.l_k + (wn * 16 * FR + f * 16 + bi) * ob.l_row];
          }
#pragma unroll
        for (int ks = 0; ks < KSB; ++ks)
#pragma unroll
          for (int fm = 0; fm < FR; ++fm)
#pragma unroll
            for (int fn = 0; fn < FR; ++fn) acc[fm][fn] = mma16x16x4(af[ks][fm], bf[ks][fn], acc[fm][fn]);
      }
      // next tile (kt+1, ring slot (s+1) % DEPTH) into the other image, then refill that slot with tile
      // kt+1+DEPTH; tiles beyond nkt are all-zero (clamped, masked loads): harmless
      const int sn = (s + 1) % DEPTH;
      store_tiles(sn, img ^ 1);
      load_tiles(sn, kbeg + (kt + 1 + DEPTH) * BK);
      lds_barrier();
    }
  }

  gemm_epilogue<FR, TF>(g, d, t, wm, wn, bi, q, tid, lane, wave, acc, tgt, do_mse);
}

static int g_cus = 0;
int device_cus() {
  if (g_cus == 0) {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
      g_cus = prop.multiProcessorCount;
    if (g_cus <= 0) g_cus = 256;
  }
  return g_cus;
}

// What one descriptor (problem i of its group) must satisfy.  has_mse: a squared-error epilogue rides on the problem and may
// stand in for its c.
static int gemm_check_problem(const MfmGemmDesc& d, int i, int precision, bool has_mse) {
  MFM_REQUIRE(d.m > 0 && d.n > 0 && d.k >= 0 && d.batch > 0, "gemm[%d]: bad dims m=%d n=%d k=%d batch=%d", i, d.m, d.n, d.k, d.batch);
  MFM_REQUIRE(d.a && d.b && (d.c || (has_mse && !d.accumulate && !d.c_bf16)), "gemm[%d]: null operand", i);
  if (d.a_bf16 || d.c_bf16) {
    MFM_REQUIRE(precision == 1, "gemm[%d]: bf16-resident operands (a_bf16 / c_bf16) are taken by the bf16 entry point only", i);
    MFM_REQUIRE(!d.c_bf16 || (!d.accumulate && d.split_k <= 1), "gemm[%d]: c_bf16 needs a plain (non-accumulating, unsplit) product", i);
    const GemmForm fa = gemm_operand_form(d.a_sm, d.a_sk);
    MFM_REQUIRE(!d.a_bf16 || ((((uintptr_t)d.a) & 15) == 0 && (d.a_sz & 7) == 0 &&
                              ((fa == GEMM_K_CONTIG && (d.a_sm & 7) == 0) || (fa == GEMM_ROW_CONTIG && (d.a_sk & 7) == 0))),
                "gemm[%d]: a_bf16 needs a unit-stride axis on 16-byte boundaries (a_sm=%lld a_sk=%lld a_sz=%lld)", i,
                (long long)d.a_sm, (long long)d.a_sk, (long long)d.a_sz);
  }
  MFM_REQUIRE(d.n_valid >= 0 && d.n_valid <= d.n, "gemm[%d]: n_valid %d > n %d", i, d.n_valid, d.n);
  MFM_REQUIRE(d.split_k <= 1 || d.accumulate, "gemm[%d]: split_k needs accumulate", i);
  // The kernels form an operand's extent (gemm_operand_bytes) and every load offset (off * 4) in BYTES in 32-bit ints:
  // the span of one batch member, first to last element, is held to what those carry, 2^31 - 1 bytes (2^29 - 1 fp32
  // elements).  Beyond it the extent wraps and the loads return zeros or another row without any error.
  const int64_t lim = ((int64_t)1 << 31) - 1;
  MFM_REQUIRE(d.a_sm >= 0 && d.a_sk >= 0 && d.b_sk >= 0 && d.b_sn >= 0 && d.a_sm <= lim && d.a_sk <= lim && d.b_sk <= lim && d.b_sn <= lim,
              "gemm[%d]: operand strides must lie in [0, 2^31) (a_sm=%lld a_sk=%lld b_sk=%lld b_sn=%lld)", i,
              (long long)d.a_sm, (long long)d.a_sk, (long long)d.b_sk, (long long)d.b_sn);
  const int64_t sa = gemm_operand_elems<int64_t>(d.m, d.k, d.a_sm, d.a_sk), ba = gemm_operand_bytes<int64_t>(d.m, d.k, d.a_sm, d.a_sk, d.a_bf16 ? 2 : 4);
  const int64_t sb = gemm_operand_elems<int64_t>(d.k, d.n_valid, d.b_sk, d.b_sn), bb = gemm_operand_bytes<int64_t>(d.k, d.n_valid, d.b_sk, d.b_sn, 4);
  MFM_REQUIRE(ba <= lim,
              "gemm[%d]: operand a spans %lld elements (%lld bytes); the 32-bit byte offsets of the tile loads hold 2^31 - 1 bytes",
              i, (long long)sa, (long long)ba);
  MFM_REQUIRE(bb <= lim,
              "gemm[%d]: operand b spans %lld elements (%lld bytes); the 32-bit byte offsets of the tile loads hold 2^31 - 1 bytes",
              i, (long long)sb, (long long)bb);
  return MFM_OK;
}

// The launch plan of a group of checked problems on a device of `cus` CUs: tile size 32 FR, kernel form (vec: no oddly
// strided operand; bf16: the bf16-operand kernel), and per problem the tiles, K split and first workgroup in g.p / g.begins.
static int gemm_plan_group(const MfmGemmDesc* descs, int count, int cus, int precision, int mse_count, GemmGroup& g, int& FR, bool& vec,
                           bool& bf16, int& total) {
  // tile size from the block count with 64x64 tiles and no split
  long blocks64 = 0;
  for (int i = 0; i < count; ++i) blocks64 += (long)cdiv(descs[i].m, 64) * cdiv(descs[i].n, 64) * descs[i].batch;
  FR = (blocks64 >= 2L * cus) ? 2 : 1;
  // 128x128 tiles (FR = 4) are opt-in: on single large forward-layout products they add ~10 % over 64x64 (fp32:
  // 61 -> 69 TF/s on the projection shape, 86 -> 99 TF/s at 4096^3), but the step's grouped launches mix in small-K
  // and weight-gradient problems that lose more than that (proj launch at B=2048: 457 -> 514 us), and the bf16-operand
  // kernel is faster at 64x64 throughout (profiles/r02_gemm_tiles.txt)
  if (const char* e = opt_get("MFM_GEMM_FR")) {      // tuning override
    FR = (e[0] == '4') ? 4 : ((e[0] == '2') ? 2 : 1);
    if (FR == 4 && mse_count > 0) FR = 2;
  }
  const int BT = 32 * FR;
  long base_blocks = 0;
  for (int i = 0; i < count; ++i)
    base_blocks += (long)cdiv(descs[i].m, BT) * cdiv(descs[i].n, BT) * descs[i].batch;
  const long kdepth = 2048;      // K elements one workgroup walks at most (accumulating problems; measured 256..4096 at B=512/2048)
  vec = true;
  for (int i = 0; i < count; ++i) {
    const MfmGemmDesc& d = descs[i];
    if (d.k == 0) continue;        // no element of a or b is part of the product (its strides are replaced below)
    if (gemm_operand_form(d.a_sm, d.a_sk) == GEMM_ODD || gemm_operand_form(d.b_sn, d.b_sk) == GEMM_ODD) vec = false;
  }
  // bf16 MFMA operands (precision 1) need every operand unit-stride along its 16-byte load groups; a group with an
  // oddly strided operand runs on the fp32 kernel's dword path instead
  bf16 = (precision == 1) && vec;
  for (int i = 0; i < count; ++i)
    MFM_REQUIRE(bf16 || !(descs[i].a_bf16 || descs[i].c_bf16), "gemm[%d]: bf16-resident operands need unit-stride operands in the whole group", i);
  const int bk = bf16 ? BKB : BK;
  for (int i = 0; i < count; ++i) {
    GemmProblem& P = g.p[i];
    P.d = descs[i];
    if (P.d.k == 0) {              // C = bias: the kernel's clamped, masked tile fetches stay on element 0 of a and b
      P.d.a_sz = P.d.a_sm = 0; P.d.a_sk = 1;
      P.d.b_sz = P.d.b_sn = 0; P.d.b_sk = 1;
    }
    P.tiles_m = cdiv(P.d.m, BT);
    P.tiles_n = cdiv(P.d.n, BT);
    int split = P.d.split_k;
    if (split <= 0) {
      // auto (accumulate problems only).  Two reasons to split K: (a) fill the chip when the whole
      // group has few blocks; (b) bound the serial K loop of ONE block -- a weight-gradient product
      // has a small output and K = T*B rows, and must not run as 10 blocks x 40960 deep just because
      // a large sibling problem already fills the grid.
      split = 1;
      if (P.d.accumulate && P.d.k >= 128) {
        const long want_fill = (3L * cus + base_blocks - 1) / base_blocks;
        const long want_depth = (P.d.k + kdepth - 1) / kdepth;
        long want = want_fill > want_depth ? want_fill : want_depth;
        const long maxs = P.d.k / 64;
        split = (int)(want < 1 ? 1 : (want > maxs ? maxs : want));
        if (split < 1) split = 1;
      }
    }
    int kps = round_up(cdiv(P.d.k > 0 ? P.d.k : 1, split), bk);
    split = cdiv(P.d.k > 0 ? P.d.k : 1, kps);
    P.d.split_k = split;
    P.k_per_split = kps;
    g.begins[i] = P.tiles_m * P.tiles_n * P.d.batch * split;
  }
  total = gemm_assign_blocks(g);
  return MFM_OK;
}

// The one place that names the instantiations: (bf16, FR, vec) -> kernel.
static int gemm_dispatch(const GemmGroup& g, bool bf16, int FR, bool vec, int total, hipStream_t stream) {
  static const GemmKernel f32[3][2] = {{gemm_f32_kernel<1, false>, gemm_f32_kernel<1, true>},
                                       {gemm_f32_kernel<2, false>, gemm_f32_kernel<2, true>},
                                       {gemm_f32_kernel<4, false>, gemm_f32_kernel<4, true>}};
  const GemmKernel kernel = bf16 ? gemm_bf16_kernel_for(FR) : f32[FR == 4 ? 2 : (FR == 2 ? 1 : 0)][vec ? 1 : 0];
  MFM_LAUNCH_TIMED(kernel, dim3(total), dim3(256), 0, stream, g);
  MFM_LAUNCH_CHECK(bf16 ? "gemm_bf16_kernel" : "gemm_f32_kernel");
  return MFM_OK;
}

// Host-side launch of one group (count <= MFM_GEMM_MAXP).
int gemm_group_launch(const MfmGemmDesc* descs, int count, hipStream_t stream, const ZeroSpans* zs, const MseEpi* mse,
                      int mse_count, int precision, const GemmEpiSet* epis) {
  MFM_REQUIRE(count >= 1 && count <= MFM_GEMM_MAXP, "gemm group: count %d out of range", count);
  GemmGroup g;
  memset(&g, 0, sizeof(g));
  g.count = count;
  MFM_REQUIRE(mse_count >= 0 && mse_count <= 3 && mse_count <= count && (mse_count == 0 || mse), "gemm group: bad mse epilogue count %d", mse_count);
  g.mse_count = mse_count;
  for (int i = 0; i < mse_count; ++i) {
    MFM_REQUIRE(mse[i].x && !descs[i].accumulate && descs[i].batch == 1, "gemm group: mse epilogue %d needs a plain (non-accumulating, unbatched) product", i);
    g.mse[i] = mse[i];
  }
  if (epis && epis->count > 0) {
    MFM_REQUIRE(epis->count <= MFM_GEMM_NEPI && epis->count <= count && epis->epi, "gemm group: %d output transforms (max %d)", epis->count, MFM_GEMM_NEPI);
    for (int i = 0; i < epis->count; ++i) {
      const GemmEpi& e = epis->epi[i];
      MFM_REQUIRE(e.kind >= 0 && e.kind <= 3 && (e.kind == 0 || e.kind == 2 || e.aux), "gemm group: bad output transform %d", i);
      MFM_REQUIRE(e.kind == 0 || (!descs[i].accumulate && descs[i].split_k <= 1 && descs[i].batch == 1),
                  "gemm group: output transform %d needs a plain (non-accumulating, unbatched) product", i);
      g.epi[i] = e;
    }
    g.epi_count = epis->count; g.epi_train = epis->train; g.epi_seed = epis->seed; g.epi_tick = epis->tick;
  }
  if (zs) {
    for (int i = 0; i < MFM_GEMM_ZSPANS; ++i) {
      if (zs->n[i] <= 0) continue;
      MFM_REQUIRE((zs->n[i] & 3) == 0 && (((uintptr_t)zs->ptr[i]) & 15) == 0, "gemm group: zero span %d not 16-byte shaped", i);
      g.zero_ptr[i] = zs->ptr[i]; g.zero_n[i] = zs->n[i];
    }
  }
  int rc, FR, total;
  bool vec, bf16;
  for (int i = 0; i < count; ++i)
    if ((rc = gemm_check_problem(descs[i], i, precision, i < mse_count)) != MFM_OK) return rc;
  if ((rc = gemm_plan_group(descs, count, device_cus(), precision, mse_count, g, FR, vec, bf16, total)) != MFM_OK) return rc;
  return gemm_dispatch(g, bf16, FR, vec, total, stream);
}

}  // namespace mfm

// the two precisions' entry points: `name` is the caller's, for its error texts
static int gemm_grouped_entry(const char* name, const MfmGemmDesc* descs, int count, void* stream, int precision) {
  if (!descs || count <= 0) {
    mfm::set_error("%s: no problems", name);
    return MFM_ERR_ARG;
  }
  for (int i = 0; i < count; ++i)       // (the library uses the reserved bytes internally: a caller's garbage there would be a device pointer)
    if (descs[i].reserved_[0] != 0 || descs[i].reserved_[1] != 0) {
      mfm::set_error("%s: problem %d has non-zero reserved_ fields (zero the struct before filling it)", name, i);
      return MFM_ERR_ARG;
    }
  int done = 0;
  while (done < count) {
    int n = count - done;
    if (n > MFM_GEMM_MAXP) n = MFM_GEMM_MAXP;
    int rc = mfm::gemm_group_launch(descs + done, n, (hipStream_t)stream, nullptr, nullptr, 0, precision);
    if (rc != MFM_OK) return rc;
    done += n;
  }
  return MFM_OK;
}

extern "C" int mfm_gemm_grouped_f32(const MfmGemmDesc* descs, int count, void* stream) {
  return gemm_grouped_entry("mfm_gemm_grouped_f32", descs, count, stream, 0);
}

extern "C" int mfm_gemm_grouped_bf16(const MfmGemmDesc* descs, int count, void* stream) {
  return gemm_grouped_entry("mfm_gemm_grouped_bf16", descs, count, stream, 1);
}

extern "C" int mfm_device_cus(void) { return mfm::device_cus(); }

