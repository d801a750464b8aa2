// Decoder output layer, forward AND backward-to-hidden in one launch (fp32 plans).
//
// Reference: decoderLSTM.fc1 applied to every decoder hidden state (mfm_model.py:40-63), the three reconstruction
// losses `lda_x* * mse(x_hat, x)` (mfm_mosi.py:441-446) and, in training, what autograd sends back through fc1 to the
// hidden states.  In the plan these were two grouped-GEMM launches on the dependency chain (F4 with the squared-error
// epilogue, B0); at the reference's B=32 each is a ~10 us launch of which most is latency.  Nothing else separates
// them: d x_hat is an elementwise function of x_hat, so a workgroup that owns 16 (t, b) rows of one decoder can run
//
//   x_hat = H Wfc^T + b  ->  diff = x_hat - x  ->  loss += sum diff^2 / count,  dx_hat = 2 lda / count * diff
//   dH    = dx_hat Wfc                                                          (training only)
//
// back to back with dx_hat staged in LDS.  Wfc is read from L2 twice (once per product), never staged: a workgroup
// uses every element exactly once per product.  The weight-gradient products dWfc = dx_hat^T H and dbfc stay in the
// step's tail GEMM launch (they only feed the optimizer).
//
// Decomposition: one workgroup = 16 rows x one group of <= 8 output fragments (16 columns each) of one decoder.  Decoder l
// (300 columns, 19 fragments) takes 3 column groups per row tile; their contributions to dH are partial sums over the
// columns and are ADDED to dH with atomics -- the caller puts the dH block into the step's zero spans.  (A single column group
// stores instead: no atomics, the same bits every time.)
//
// 512 threads = 8 waves; MFMA 16x16x4 fp32 tiles.  Both products have the same shape:
//   product 1: wave w owns output fragment w of the group; the reduction over hidden units walks 16-wide blocks: lane
//              (bi, q) takes the four units 16 j + 4 q + {0..3} of its row of H (LDS, one 16-byte read) and of row
//              n = bi of Wfc (one 16-byte buffer load) and feeds four MFMAs, one into each of four independent accumulators
//              -- the order of the reduction index inside a block is free as long as both operands agree.
//   product 2: wave w owns output fragment w of dH (16 hidden units) over the WHOLE column range of the group, so no two
//              waves hold parts of one element and dH leaves straight from the accumulators.  Its weight operand is the
//              transpose of product 1's: the group's slice of Wfc is read from memory ONCE -- every wave parks the weight
//              registers of product 1 in LDS transposed (Wt[unit][column], behind the MFMAs' issue), and product 2 reads
//              lane (bi, q)'s four columns 16 j + 4 q + {0..3} of unit row bi with one 16-byte LDS read, next to the same
//              four columns of d x_hat.  (Before: a second, 4-byte strided fetch of Wfc -- 32 requests per lane in front of
//              the targets and the bias in the in-order return queue --, the reduction over the columns split over the
//              waves, and the eight partial tiles summed through LDS: write, barrier, add, barrier, sum.)
//   One barrier separates the products (d x_hat, the parked weights and the waves' loss sums become visible together); the
//   loss slot, x_hat and d x_hat leave behind product 2's issue.  Every global operand is requested before the first MFMA, in
//   the order it is needed: H, weights, targets, bias.
#include <hip/hip_runtime.h>
#include <atomic>
#include "internal.h"
#include "lstamp.h"

namespace mfm {

constexpr int FC1_THREADS = 512;
constexpr int FC1_WAVES = 8;
constexpr int FC1_ROWS = 16;
constexpr int FC1_MAXF = 8;                  // Hp <= 128; <= 8 output fragments per column group
constexpr int FC1_LD = 16 * FC1_MAXF + 4;    // LDS row stride: (LD / 4) odd and LD == 4 (mod 64): conflict-free 16-byte row reads,
                                             // and 4 LD == 16 (mod 32): the transposed 4-byte writes of a half wave hit 32 banks
constexpr int FC1_OOB = 0x7FFFFFF0;          // buffer offset beyond any resource: the load returns 0

// bf16 plans: the same products with every operand (H, Wfc, dx_hat) rounded to bf16 first and fp32 accumulation -- what
// the bf16-operand GEMM computes; at these sizes the launch is latency, not matrix time, so the fp32 MFMA stays
__device__ __forceinline__ float rnd_bf16(float x, bool on) { return on ? (float)(__bf16)x : x; }

__global__ __launch_bounds__(FC1_THREADS) void dec_fc1_kernel(const DecFc1Launch L) {
  __shared__ __attribute__((aligned(16))) float Ht[FC1_ROWS * FC1_LD];              // hidden rows
  __shared__ __attribute__((aligned(16))) float Dx[FC1_ROWS * FC1_LD];              // d x_hat of this column group
  __shared__ float red[FC1_WAVES];
  extern __shared__ __attribute__((aligned(16))) float Wt[];                        // training: [max Hp][FC1_LD], Wfc^T of the group
  LSTAMP(2, 0);
  // which decoder, row tile, column group
  int m = 0;
#pragma unroll
  for (int i = 1; i < 3; ++i)
    if (i < L.n_items && (int)blockIdx.x >= L.it[i].tile_begin) m = i;
  const DecFc1Item& I = L.it[m];
  const int d = I.d, h = I.h, Hp = I.Hp;
  const int local = (int)blockIdx.x - I.tile_begin;
  const int cg = local % I.col_groups;
  const int row0 = (local / I.col_groups) * FC1_ROWS;
  const int NF1 = (d + 15) >> 4;
  const int f0 = cg * I.frags_per_group, nfw = min(I.frags_per_group, NF1 - f0);      // this group's fragments
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bi = lane & 15, q = lane >> 4;
  const int J = Hp >> 4;                          // 16-wide reduction blocks of product 1 == output fragments of product 2
  const bool bwd = L.with_bwd != 0;

  // ---- requests.  The 16 hidden rows (pad units of the saved states are exact zeros): one 16-byte piece per thread
  const int per_row = Hp >> 2;                    // 16 * per_row <= 512
  const int hr = tid / per_row, hk = (tid - hr * per_row) << 2;
  f32x4 hreg = f32x4{0.f, 0.f, 0.f, 0.f};
  if (hr < FC1_ROWS && row0 + hr < L.rows) hreg = *reinterpret_cast<const f32x4*>(I.hs + (int64_t)(row0 + hr) * Hp + hk);
  const __amdgpu_buffer_rsrc_t wres = __builtin_amdgcn_make_buffer_rsrc((void*)I.w, 0, d * h * 4, 0x00020000);
  const int n = (f0 + wave) * 16 + bi;            // this lane's output column in product 1
  const bool cok = (int)(wave < nfw) & (int)(n < d);
  f32x4 w1[FC1_MAXF];                             // (unconditional: blocks >= J and masked columns ask outside the resource)
#pragma unroll
  for (int j = 0; j < FC1_MAXF; ++j) {
    const bool ok = (int)cok & (int)(j < J);
    w1[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wres, ok ? (n * h + 16 * j + 4 * q) * 4 : FC1_OOB, 0, 0));
  }
  float xv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * q + r;
    xv[r] = (cok && row < L.rows) ? I.x[(int64_t)row * I.ldx + n] : 0.0f;
  }
  const float bv = cok ? I.bias[n] : 0.0f;
  const bool rb = L.bf16 != 0;
  if (rb) {
#pragma unroll
    for (int e = 0; e < 4; ++e) hreg[e] = rnd_bf16(hreg[e], true);
  }
  if (hr < FC1_ROWS) *reinterpret_cast<f32x4*>(Ht + hr * FC1_LD + hk) = hreg;
  lds_barrier();
  LSTAMP(2, 1);
  LSTAMP_V(2, 10, 5);                             // (behind the weights: 4 target loads + the bias; a tile with fewer than 4 valid
                                                  //  rows per lane group issues fewer, and the stamp then comes early: full tiles only)

  // ---- product 1 (units >= h of a weight row belong to the next row -- finite values -- and meet zeros of the hidden tile).
  //      Waves beyond the group's fragments have nothing to do until product 2: the columns they would own are never read.
  f32x4 acc1[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) acc1[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  float xh[4] = {0.f, 0.f, 0.f, 0.f}, dxr[4] = {0.f, 0.f, 0.f, 0.f};
  float lsum = 0.0f;
  if (wave < nfw) {
#pragma unroll
    for (int j = 0; j < FC1_MAXF; ++j) {
      if (j < J) {                                // (uniform)
        const f32x4 hv = *reinterpret_cast<const f32x4*>(Ht + bi * FC1_LD + 16 * j + 4 * q);
        f32x4 wv;
#pragma unroll
        for (int e = 0; e < 4; ++e) wv[e] = rnd_bf16(w1[j][e], rb);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc1[e] = mma16x16x4(hv[e], wv[e], acc1[e]);
        if (bwd) {
          // product 2's operand: Wt[unit][column of the group], pad units zero (they must come out of dH as exact zeros)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int u = 16 * j + 4 * q + e;
            Wt[u * FC1_LD + wave * 16 + bi] = u < h ? wv[e] : 0.0f;
          }
        }
      }
    }
    LSTAMP_W(2, 11);
    // ---- squared-error epilogue
    const f32x4 s1 = (acc1[0] + acc1[1]) + (acc1[2] + acc1[3]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * q + r;
      xh[r] = s1[r] + bv;
      dxr[r] = 0.0f;
      if (cok && row0 + row < L.rows) {
        const float diff = xh[r] - xv[r];
        lsum = fmaf(diff, diff, lsum);
        dxr[r] = I.grad_scale * diff;
      }
      Dx[row * FC1_LD + wave * 16 + bi] = rnd_bf16(dxr[r], rb);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) lsum += __shfl_xor(lsum, o, 64);
  if (lane == 0) red[wave] = lsum;
  LSTAMP(2, 12);
  lds_barrier();
  LSTAMP(2, 2);

  // ---- product 2: dH[16, fragment `wave`] (+)= dx_hat[16, group columns] Wfc[group columns, fragment `wave`]
  f32x4 acc2[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) acc2[e] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool w2on = (int)bwd & (int)(wave < J);
  if (w2on) {
    f32x4 av[FC1_MAXF], wv[FC1_MAXF];
#pragma unroll
    for (int j = 0; j < FC1_MAXF; ++j) {
      if (j < nfw) {                              // (uniform)
        av[j] = *reinterpret_cast<const f32x4*>(Dx + bi * FC1_LD + 16 * j + 4 * q);
        wv[j] = *reinterpret_cast<const f32x4*>(Wt + (wave * 16 + bi) * FC1_LD + 16 * j + 4 * q);
      }
    }
#pragma unroll
    for (int j = 0; j < FC1_MAXF; ++j) {
      if (j < nfw) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc2[e] = mma16x16x4(av[j][e], wv[j][e], acc2[e]);
      }
    }
  }
  // ---- behind product 2's issue: x_hat and d x_hat, the loss slot (the last wave: the one without a dH fragment unless Hp = 128)
  if (cok) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * q + r;
      if (row < L.rows) {
        const int64_t o = (int64_t)row * d + n;
        if (I.xhat) I.xhat[o] = xh[r];
        if (I.dxhat) I.dxhat[o] = dxr[r];
      }
    }
  }
  if (tid == FC1_THREADS - 64 && I.loss) {
    float s = 0.0f;
#pragma unroll
    for (int w = 0; w < FC1_WAVES; ++w) s += red[w];
    atomicAdd(I.loss, s * I.inv_count);
  }
  if (w2on) {
    const f32x4 s2 = (acc2[0] + acc2[1]) + (acc2[2] + acc2[3]);      // pad units: exact zeros (zero rows of Wt)
    float* o = I.dhs + (int64_t)(row0 + 4 * q) * Hp + wave * 16 + bi;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (row0 + 4 * q + r < L.rows) {
        if (I.col_groups == 1) o[r * Hp] = s2[r];
        else atomicAdd(o + r * Hp, s2[r]);
      }
    }
  }
  LSTAMP(2, 13);
  LSTAMP_W(2, 15);
}

// MFM_ERR_UNSUPPORTED: a shape this kernel does not take (the caller falls back to the two GEMM launches)
// `dhs_zeroed`: the caller has put the dH buffers into the step's zero spans (required for more than one column group)
int dec_fc1_launch(DecFc1Launch& L, bool dhs_zeroed, hipStream_t stream) {
  MFM_REQUIRE(L.n_items >= 1 && L.n_items <= 3 && L.rows >= 1, "dec fc1: bad launch");
  int tiles = 0;
  const int row_tiles = (L.rows + FC1_ROWS - 1) / FC1_ROWS;
  for (int i = 0; i < L.n_items; ++i) {
    DecFc1Item& I = L.it[i];
    MFM_REQUIRE(I.hs && I.w && I.bias && I.x && I.d >= 1 && I.h >= 1 && I.Hp >= I.h && (I.Hp & 15) == 0, "dec fc1: item %d", i);
    MFM_REQUIRE(!L.with_bwd || I.dhs, "dec fc1: item %d: backward without a dH buffer", i);
    if (I.Hp > 16 * FC1_MAXF || (int64_t)I.d * I.h >= ((int64_t)1 << 28)) return MFM_ERR_UNSUPPORTED;
    const int NF1 = (I.d + 15) >> 4;
    // (rounds 3-5: 5 fragments per group, "spread the columns" -- decoder l on 160 workgroups.  Round 6, the launch clock: the
    // partial dH tiles of a row tile's column groups are added with memory-side atomics, and those, not the products, end the
    // launch: the single-group tiles of the narrow decoders leave 2.4 us after their first product, the four-group tiles 3.9
    // (median) to 5.4 us.  Step time against fragments per group: 3 0.1484, 4 0.1467, 5 0.1454, 7 0.1453, 8 0.1442 ms; ten waves
    // with groups of 10 were built and are slower, 0.1467.)
    if (NF1 > FC1_MAXF && !(dhs_zeroed || !L.with_bwd)) return MFM_ERR_UNSUPPORTED;      // several groups add into dH
    I.frags_per_group = std::min(FC1_MAXF, NF1);
    I.col_groups = (NF1 + I.frags_per_group - 1) / I.frags_per_group;
    I.tile_begin = tiles;
    tiles += row_tiles * I.col_groups;
  }
  // the transposed weight slice of product 2: [max Hp][FC1_LD] floats behind the static tiles (up to 66 KB at Hp = 128)
  int max_hp = 0;
  for (int i = 0; i < L.n_items; ++i) max_hp = std::max(max_hp, L.it[i].Hp);
  const size_t smem = L.with_bwd ? (size_t)max_hp * FC1_LD * sizeof(float) : 0;
  // (the attribute belongs to the device's copy of the kernel: once per device, from whichever thread comes first)
  static std::atomic<unsigned long long> lds_attr_set{0};
  int dev = 0;
  MFM_HIP_CHECK(hipGetDevice(&dev));
  const unsigned long long dev_bit = 1ull << (dev & 63);
  if (!(lds_attr_set.load(std::memory_order_acquire) & dev_bit)) {
    MFM_HIP_CHECK(hipFuncSetAttribute((const void*)dec_fc1_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 16 * FC1_MAXF * FC1_LD * (int)sizeof(float)));
    lds_attr_set.fetch_or(dev_bit, std::memory_order_release);
  }
  LSTAMP_BIND();
  MFM_LAUNCH_TIMED(dec_fc1_kernel, dim3(tiles), dim3(FC1_THREADS), smem, stream, L);
  MFM_LAUNCH_CHECK("dec_fc1_kernel");
  return MFM_OK;
}

}  // namespace mfm

extern "C" int mfm_dec_fc1_f32(const MfmDecFc1Item* items, int32_t count, int32_t rows, int32_t with_bwd, int32_t bf16_operands,
                               int32_t dhs_zeroed, void* stream) {
  MFM_REQUIRE(items && count >= 1 && count <= 3, "dec fc1: 1..3 items");
  mfm::DecFc1Launch L;
  memset(&L, 0, sizeof(L));
  L.n_items = count; L.rows = rows; L.with_bwd = with_bwd ? 1 : 0; L.bf16 = bf16_operands ? 1 : 0;
  for (int i = 0; i < count; ++i) {
    mfm::DecFc1Item& I = L.it[i];
    const MfmDecFc1Item& s = items[i];
    I.hs = s.hs; I.w = s.w; I.bias = s.bias; I.x = s.x; I.ldx = s.ldx;
    I.xhat = s.xhat; I.dxhat = s.dxhat; I.dhs = s.dhs; I.loss = s.loss;
    I.d = s.d; I.h = s.h; I.Hp = s.Hp; I.inv_count = s.inv_count; I.grad_scale = s.grad_scale;
  }
  return mfm::dec_fc1_launch(L, dhs_zeroed != 0, (hipStream_t)stream);
}
