// What the inference launches built on small_fwd_body<.., REC = false> share (predict.hip, generate.hip, impute.hip,
// objective.hip, zeros.hip).  Device: a tile's rows into LDS and back out.  Host: the sizing rules (chunk rows, tile rows, the LDS the recurrence lays out), the
// refusals and argument checks, the SeqDev of an LSTM, the grouped GEMMs around the recurrence, and the two launch rules.
//
// The launch rules: a kernel that runs several LSTMs in one launch picks its body per block with a switch, and that switch is
// instantiated for the canonical size tuples only (the rule of lstm_seq_small.hip: a switch over all sizes costs the register
// allocation of every body).  Any other size combination takes one launch per LSTM of the same kernel, instantiated for that
// LSTM's size alone (infer_launch_tuple_or_each, infer_launch_hk4).
#pragma once
#include <algorithm>
#include <type_traits>

#include "lstm_seq_small_dev.h"
#include "dense_rows_dev.h"

namespace mfm {

// rows [b0, b0 + R) of z [n, zs] -> LDS [zs][R]; rows beyond n: zeros
template <int R>
__device__ __forceinline__ void stage_rows(const float* __restrict__ z, const int zs, const int b0, const int n, float* out) {
  for (int e = threadIdx.x; e < zs * R; e += blockDim.x) {
    const int r = e / zs, k = e - r * zs;
    out[k * R + r] = (b0 + r < n) ? z[(int64_t)(b0 + r) * zs + k] : 0.0f;
  }
  lds_barrier();
}

// the way back: LDS [w][R] -> rows [b0, b0 + R) of dst [n, w]; rows beyond n are not written.  tid: threadIdx.x as the kernel
// read it at its top -- a second read here, behind the per-block switch, cost six encoder instantiations 16 bytes of scratch
template <int R>
__device__ __forceinline__ void store_rows(const float* act, float* dst, const int w, const int b0, const int n, const int tid) {
  for (int e = tid; e < w * R; e += blockDim.x) {
    const int r = e / w, o = e - r * w;
    if (b0 + r < n) dst[(int64_t)(b0 + r) * w + o] = act[o * R + r];
  }
}

// ---------------------------------------------------------------- the decoders' launch (generate.hip; impute.hip launches it too)
#define INFER_DEC 3
struct DecOne {
  SeqDev seq;                                  // w_ih, w_hh, b_ih, b_hh, h = fy + fm, Hp, hk4, is_dec; hs: this chunk's [T, n, Hp]
  const float* w[2]; const float* b[2];        // z_m -> f_m: fc1, fc2
  const float* zm; const float* zy;            // this chunk's rows [n, zs] / [n, zys]
  float* y_hat;                                // this chunk's rows [n, od]; null: this decoder's workgroups skip the classifier
  int zs, fm, block_begin;
};
struct DecodeDev {
  DecOne d[INFER_DEC];
  const float* wy[4]; const float* by[4];      // zy_to_fy fc1, fc2, fy_to_y fc1, fc2
  int count, T, n, zys, fy, od, maxw, seq_floats;
};
// decode_factors_kernel on one chunk of P.n rows in tiles of R (1 or 4) rows; P.d[0 .. P.count) filled but for block_begin.  The
// kernel's instantiations stay in generate.hip alone
int decode_factors_launch(const char* who, DecodeDev& P, int R, int threads, size_t lds_bytes, hipStream_t stream);

// ---------------------------------------------------------------- the decoders' fc1 fused with the squared error (objective.hip; zeros.hip launches it too)
#define OBJ_BM 64          // rows of h per workgroup: 4 waves x 16
#define OBJ_BN 64          // columns of x_hat per workgroup: up to 4 fragments of 16 per wave
#define OBJ_THREADS 256
struct Fc1SqItem {
  const float* hs; const float* w; const float* bias;      // H [M, Hp] (the chunk's [T, n, Hp]), W_fc1 [d, h], b [d]
  const float* x;                                          // x[0][n0][first column of m]: chunk row (t, i) at ((int64)t N + i) D
  float* partials;                                         // one slot per workgroup of this item
  int d, h, Hp, col_tiles, tile_begin;
};
struct Fc1SqDev { Fc1SqItem it[INFER_DEC]; int64_t N; int M, n, D; };
// workgroups (= partial slots) of fc1_sqerr_kernel over a chunk of n rows; dm: the three decoders' output widths
static int64_t fc1_sqerr_tiles(int64_t T, int64_t n, const int32_t* dm) {
  int64_t t = 0;
  for (int m = 0; m < INFER_DEC; ++m) t += ((T * n + OBJ_BM - 1) / OBJ_BM) * ((dm[m] + OBJ_BN - 1) / OBJ_BN);
  return t;
}
// the launch chunk by chunk, behind decode_factors_prepare (below), whose DecLaunch names T, the chunk rows and the d_m.
// prepare: what does not depend on the chunk -- the decoders' stored h and fc1 into F, the widest h, the column of each modality
// in x, 1 / (T N d_m) of the WHOLE split -- and the check that a chunk's workgroups can be counted with 32 bits.  The kernel
// stays in objective.hip alone
struct DecLaunch;
struct Fc1SqLaunch { Fc1SqDev F; int T, hmax, col[INFER_DEC]; double inv_gen[INFER_DEC]; };
int fc1_sqerr_prepare(const char* who, const DecLaunch& L, int64_t N, Fc1SqLaunch& S);
// x: the whole split [T, N, D], the chunk its rows [n0, n0 + n); one partial per workgroup from `partials` on: modality m's
// are the npart[m] floats at part[m]
int fc1_sqerr_chunk(Fc1SqLaunch& S, const float* x, int64_t n0, int n, float* partials, const float** part, int* npart, hipStream_t stream);

// sum over a workgroup of OBJ_THREADS in a fixed order; every thread returns it
__device__ __forceinline__ double finish_sum(double v, double* red, const int tid) {
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = OBJ_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// this thread's part of a chunk's label loss: |y_hat - y| over [n, od] (loss_kind 0), or logsumexp - picked per row as in
// predict.hip (1); thread-strided over a workgroup of OBJ_THREADS
__device__ __forceinline__ double label_loss_part(const float* y_hat, const void* y, const int n, const int od, const int loss_kind,
                                                  const int tid) {
  double disc = 0.0;
  if (loss_kind == 0) {
    const float* yt = reinterpret_cast<const float*>(y);
    for (int i = tid; i < n * od; i += OBJ_THREADS) disc += (double)fabsf(y_hat[i] - yt[i]);
  } else {
    const int64_t* lab = reinterpret_cast<const int64_t*>(y);
    for (int r = tid; r < n; r += OBJ_THREADS) {
      const float* yr = y_hat + (int64_t)r * od;
      float mx = yr[0];
      for (int o = 1; o < od; ++o) mx = fmaxf(mx, yr[o]);
      float se = 0.0f;
      for (int o = 0; o < od; ++o) se += expf(yr[o] - mx);
      const int lc = (int)min(max(lab[r], (int64_t)0), (int64_t)(od - 1));      // (a label outside [0, od) must not index outside y_hat)
      disc += (double)((logf(se) + mx) - yr[lc]);
    }
  }
  return disc;
}

// ---------------------------------------------------------------- the finish of the objective (objective.hip; objective_mfn.hip launches it too)
#define OBJ_ACC 5          // squared errors l, a, v; KLD sum; label-loss sum
struct ObjFinishDev {
  const float* part[INFER_DEC]; int npart[INFER_DEC];      // this chunk's squared-error partials
  const float* mu[4]; const float* lv[4]; int nz[4];       // this chunk's factors, n * size elements each (0: no KLD term)
  const float* y_hat; const void* y;                       // this chunk's [n, od] and labels
  double* acc;                                             // OBJ_ACC running sums over the chunks so far
  float* out;                                              // loss, disc, gen_l, gen_a, gen_v, reg
  double inv_gen[INFER_DEC], inv_disc;                     // 1 / (T N d_m), 1 / (N od) (L1) or 1 / N (CE): the WHOLE split
  float lda[4];                                            // lda_xl, lda_xa, lda_xv, lda_mmd
  int n, od, loss_kind, first, last;                       // last 0 on every chunk: acc is left for the caller's own finish
};
// objective_finish_kernel, one workgroup: the chunk's sums in a fixed order in fp64 into acc (the first chunk stores, the others
// add); behind the last chunk the six floats, reg = -0.5 * the KLD sum.  The kernel stays in objective.hip alone
int objective_finish_launch(const ObjFinishDev& Q, hipStream_t stream);

// ---------------------------------------------------------------- the finish of the zeroed-modality protocol (zeros.hip; zeros_mfn.hip launches it too)
#define ZER_CASES INFER_DEC
#define ZER_ACC (2 * ZER_CASES)        // squared errors l, a, v; label-loss sums of the cases no l, no a, no v
struct ZerFinishDev {
  const float* part[ZER_CASES]; int npart[ZER_CASES];      // this chunk's squared-error partials
  const float* y_hat[ZER_CASES]; const void* y;            // this chunk's [n, od] per case and its labels (null: no label loss)
  double* acc;                                             // ZER_ACC running sums over the chunks so far
  float* gen; float* disc;                                 // 3 floats each; disc null without labels
  double inv_gen[ZER_CASES], inv_disc;                     // 1 / (T N d_m), 1 / (N od) (L1) or 1 / N (CE): the WHOLE split
  int n, od, loss_kind, first, last;
};
// zeros_finish_kernel, one workgroup: the chunk's sums in a fixed order in fp64 into acc (the first chunk stores, the others
// add); behind the last chunk gen and disc.  The kernel stays in zeros.hip alone
int zeros_finish_launch(const ZerFinishDev& Q, hipStream_t stream);

// ---------------------------------------------------------------- the encoders' launch (generate.hip)
#define INFER_ENC 4
struct EncOne {
  SeqDev seq;                                  // gates (the x-projections, read only), w_hh, h, Hp, hk4
  const float* w[3]; const float* b[3];        // fc1, the mean head, the logvar head
  float* mu; float* lv;                        // this chunk's rows [n, zs]
  int zs, block_begin;
};
struct EncodeDev { EncOne d[INFER_ENC]; int count, T, n, maxw; };

// ---------------------------------------------------------------- the two halves chunk by chunk (generate.hip; objective.hip walks them too)
// prepare: the checks behind the caller's own argument checks (row cap, offsets, the refusals), then everything of the launches
// that does not depend on the chunk; workspace: *_ws_floats below.  chunk: the launches of one chunk of n <= rows rows
struct EncLaunch { EncodeDev P; int R, threads, rows, D, dd[INFER_ENC], col[INFER_ENC]; size_t lds_bytes; };
struct DecLaunch { DecodeDev P; int R, threads, rows, dm[INFER_DEC]; size_t lds_bytes; const float* fcw[INFER_DEC]; const float* fcb[INFER_DEC]; };
int encode_klef_prepare(const char* who, int T, int64_t N, int d_l, int d_a, int d_v, int zl, int za, int zv, int zy, const float* params,
                        const int64_t* offs, float* ws, int64_t max_rows, EncLaunch& L);
// x: the whole split [T, N, D], the chunk its rows [n0, n0 + n); out: the chunk's first rows of the four means, then the four logvars
int encode_klef_chunk(EncLaunch& L, const float* x, int64_t N, int64_t n0, int n, float* const* out, hipStream_t stream);
int decode_factors_prepare(const char* who, int T, int64_t N, const int32_t* sz, const float* params, const int64_t* offs, float* ws,
                           int64_t max_rows, DecLaunch& L);
// z: the chunk's first rows of zl, za, zv, zy; y_hat: the chunk's.  The recurrence launch alone: h_t is left in P.d[m].seq.hs [T, n, Hp]
int decode_factors_chunk(const char* who, DecLaunch& L, const float* const* z, float* y_hat, int n, hipStream_t stream);

// ---------------------------------------------------------------- the surrogate encoders of an observed pair (impute.hip; missing.hip launches them too)
#define IMP_CASES INFER_DEC
#define IMP_ENC (2 * IMP_CASES)
#define IMP_CASE_PTRS 22     // per case: 6 of the encoder -> z_m, 6 of the encoder -> zy, 4 of z{m}_to_f{m}, 6 of decoder_m
#define IMP_NPARAM (IMP_CASES * IMP_CASE_PTRS + 8)

struct ImpEnc {
  SeqDev seq;                                  // gates (the x-projections, read only), w_hh, h, Hp, hk4
  const float* w; const float* b;              // fc1
  float* z;                                    // this chunk's rows [n, h]
  int block_begin;
};
struct ImpEncodeDev { ImpEnc d[IMP_ENC]; int count, T, n, maxw; };

// out_c [T * n, ld_c] <- rows [n0, n0 + n) of x [T, N, D], columns s0 .. s0 + len0 - 1 then s1 .. up to k_c in all; [k_c, ld_c): zeros
struct ImpGather {
  const float* x; float* out[IMP_CASES];
  int s0[IMP_CASES], len0[IMP_CASES], s1[IMP_CASES], k[IMP_CASES], ld[IMP_CASES];
  int64_t N, n0;
  int n, T, D;
};

// the sizes of a call, from the 12 the caller passes: zl, za, zv, zy, fl, fa, fv, fy, d_l, d_a, d_v, output_dim
struct ImpSizes {
  int z[IMP_CASES], zy, fm[IMP_CASES], fy, dm[IMP_CASES], od, D;
  int din[IMP_CASES], ld[IMP_CASES];           // the observed pair of case m: its width, and the row length of its gathered copy
  int cs[IMP_CASES], nc;                       // the cases asked for, ascending
};
// false: a size below 1, or cases not one of 1, 2, 4, 7
bool imp_sizes(const int32_t* sz, int cases, ImpSizes& S);
// slot c of G (out / k / ld / s0 / len0 / s1) for the observed pair of case m, copied to `out`
void imp_gather_case(ImpGather& G, int c, int m, const ImpSizes& S, float* out);
// impute_gather_kernel over the nc slots of G (x, N, n0, n, T, D set).  The kernel stays in impute.hip alone
int impute_gather_launch(const ImpGather& G, int nc, hipStream_t stream);
// impute_encode_kernel on one chunk of P.n rows in tiles of R (1 or 4) rows; P.d[0 .. P.count) filled but for block_begin.  pairs:
// P.d holds the encoders -> z_m and -> zy of every case asked for, two per case (canonical 32 / 8 / 80 and 32); else one per case, the
// encoder -> z_m alone.  m0: the case when it is one.  The kernel's instantiations stay in impute.hip alone
int impute_encode_launch(const char* who, ImpEncodeDev& P, bool pairs, int m0, int R, int threads, size_t lds_bytes, hipStream_t stream);

// ---------------------------------------------------------------- host: sizes
static int64_t gen_rows(int64_t N, int64_t max_rows) { return (max_rows > 0 && max_rows < N) ? max_rows : N; }
static int64_t hp_of(int64_t h) { return (h + 15) / 16 * 16; }
// a part of a workspace, in floats: a multiple of 4, so that the next part is 16-byte aligned
static int64_t up4(int64_t v) { return (v + 3) / 4 * 4; }
static int64_t encode_ws_floats(int64_t T, int64_t N, int64_t zl, int64_t za, int64_t zv, int64_t max_rows) {
  return gen_rows(N, max_rows) * T * 4 * (hp_of(zl) + hp_of(za) + hp_of(zv) + hp_of(zl + za + zv));
}
static int64_t decode_ws_floats(int64_t T, int64_t N, int64_t fy, int64_t fl, int64_t fa, int64_t fv, int64_t max_rows) {
  return gen_rows(N, max_rows) * T * (hp_of(fy + fl) + hp_of(fy + fa) + hp_of(fy + fv));
}

// floats of LDS small_fwd_body<KQ, R> lays out for hidden size h (its two h buffers, then the weight staging panel / its record
// and x-projection buffers, layout kept), a multiple of 4
static size_t seq_lds_floats(int h, int R) {
  const size_t HKB = (size_t)round_up(4 * round_up(cdiv(h, 4), 2), 16);
  const size_t hh = (R == 1 && (h & 3) == 0) ? 0 : (size_t)h * h;
  const size_t rec = (2 * 6 + 2 * 4) * HKB * R;
  return (2 * HKB * R + std::max(2 * hh, rec) + 3) / 4 * 4;
}
// the same for an encoder workgroup that keeps the two h buffers and puts `nact` activations [maxw][R] of its heads behind them
static size_t enc_lds_floats(int h, int R, int nact, int maxw) {
  return std::max(seq_lds_floats(h, R), (size_t)2 * round_up(h, 16) * R + (size_t)nact * maxw * R);
}
static size_t lds_bytes_of(size_t floats) { return (floats * sizeof(float) + 15) / 16 * 16; }

static int gen_hk4(int h) { return round_up(cdiv(h, 4), 2); }

// one-row tiles below 6 workgroups per CU over the whole launch (the rule of the training recurrences), else four-row tiles
static int gen_tile_rows(int lstms, int rows) { return ((long)lstms * rows < 6L * device_cus()) ? 1 : 4; }

static void seq_fill(SeqDev& s, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int h, int is_dec) {
  s.w_ih = w_ih; s.w_hh = w_hh; s.b_ih = b_ih; s.b_hh = b_hh;
  s.h = h; s.Hp = round_up(h, 16); s.hk4 = gen_hk4(h); s.is_dec = is_dec;
}

// ---------------------------------------------------------------- host: labels
// the labels of rows n0 on: y [N, od] floats (loss_kind 0) or [N] int64 class indices (1); null stays null
static const void* labels_at(const void* y, int loss_kind, int64_t n0, int od) {
  if (!y) return nullptr;
  return loss_kind == 0 ? (const void*)(reinterpret_cast<const float*>(y) + n0 * od) : (const void*)(reinterpret_cast<const int64_t*>(y) + n0);
}
// what turns the label-loss sum of a whole split into its mean: 1 / (N od) (L1) or 1 / N (CE)
static double inv_label_count(int loss_kind, int64_t N, int od) {
  return loss_kind == 0 ? 1.0 / ((double)N * (double)od) : 1.0 / (double)N;
}

// ---------------------------------------------------------------- host: checks (MFM_OK, or the error set and its code)
// T, N and the twelve sizes of a size array (zl, za, zv, zy, fl, fa, fv, fy, d_l, d_a, d_v, output_dim)
static int infer_check_sizes(const char* who, int T, int64_t N, const int32_t* sz) {
  MFM_REQUIRE(T >= 1 && N >= 1, "%s: sizes must be positive (T %d, N %lld)", who, T, (long long)N);
  for (int i = 0; i < 12; ++i) MFM_REQUIRE(sz[i] >= 1, "%s: sizes must be positive (size %d is %d)", who, i, sz[i]);
  return MFM_OK;
}
static int infer_check_loss_kind(const char* who, int loss_kind) {
  MFM_REQUIRE(loss_kind == 0 || loss_kind == 1, "%s: unknown loss kind %d (0 = L1, 1 = cross entropy)", who, loss_kind);
  return MFM_OK;
}
// x: any contiguous float view (a batch of a [nb, T, B, D] dataset, a time crop).  Every read of it is a dword read or a
// buffer_load_dwordx4 of the grouped GEMM, which takes dword-aligned addresses: with an odd D the rows of an aligned x are
// off 16 bytes already.  params and the workspace feed 16-byte vector loads (LSTM weights, gates)
static int infer_check_aligned(const char* who, const void* params, const void* x, const void* ws) {
  MFM_REQUIRE(((uintptr_t)x & 3) == 0, "%s: x must be 4-byte aligned", who);
  MFM_REQUIRE((((uintptr_t)params | (uintptr_t)ws) & 15) == 0, "%s: params and workspace must be 16-byte aligned", who);
  return MFM_OK;
}
// `count` parameter offsets; those in [lstm_begin, lstm_end) come in groups of `period`, an LSTM's weight_ih and weight_hh first
static int infer_check_offsets(const char* who, const int64_t* offs, int count, int period, int lstm_begin = 0, int lstm_end = 1 << 30) {
  for (int i = 0; i < count; ++i) {
    const bool lstm_w = i >= lstm_begin && i < lstm_end && (i - lstm_begin) % period < 2;
    MFM_REQUIRE(offs[i] >= 0 && (!lstm_w || (offs[i] & 3) == 0), "%s: parameter offset %d is %lld (not negative; the LSTM weights 16-byte aligned)",
                who, i, (long long)offs[i]);
  }
  return MFM_OK;
}
static int infer_check_rows(const char* who, int64_t N, int64_t max_rows) {
  MFM_REQUIRE(max_rows >= 0, "%s: row cap %lld (0 = the whole split in one chunk)", who, (long long)max_rows);
  MFM_REQUIRE(N < ((int64_t)1 << 24), "%s: N = %lld rows (at most 2^24 - 1)", who, (long long)N);
  return MFM_OK;
}
// what the on-chip recurrence does not cover is refused: the caller composes the granular operations (the training forward) instead
static int infer_check_resident(const char* who, int h) {
  if (h <= MFM_SEQ_MAX_RESIDENT_H) return MFM_OK;
  set_error("%s: hidden size h = %d is beyond the register-resident recurrence (at most %d)", who, h, MFM_SEQ_MAX_RESIDENT_H);
  return MFM_ERR_UNSUPPORTED;
}
// h: named in front of the widest layer when not 0
static int infer_check_lds(const char* who, size_t lds_bytes, int maxw, int R, int h = 0) {
  if (lds_bytes <= 160 * 1024) return MFM_OK;
  char hs[24] = "";
  if (h) snprintf(hs, sizeof(hs), "h = %d, ", h);
  set_error("%s: %zu bytes of LDS per workgroup (%swidest layer %d, %d rows per workgroup) exceed the 160 KB of a CU", who, lds_bytes, hs, maxw, R);
  return MFM_ERR_UNSUPPORTED;
}
// the GEMMs index a chunk's operands with 32 bits; width: the widest row among them; what: "projection" / "product"
static int infer_check_chunk(const char* who, int rows, int T, int64_t width, const char* what) {
  MFM_REQUIRE((int64_t)rows * T * width < ((int64_t)1 << 31), "%s: a chunk of %d rows x %d steps is too large for one %s; pass a row cap",
              who, rows, T, what);
  return MFM_OK;
}

// ---------------------------------------------------------------- host: the grouped GEMMs
// grouped GEMM over `nprob` problems, MFM_GEMM_MAXP at a time; fill(p, desc) describes problem p on a zeroed descriptor
template <class F>
static int gemm_group_each(int nprob, hipStream_t stream, F fill) {
  MfmGemmDesc g[MFM_GEMM_MAXP];
  for (int p0 = 0; p0 < nprob; p0 += MFM_GEMM_MAXP) {
    const int cnt = std::min(MFM_GEMM_MAXP, nprob - p0);
    memset(g, 0, sizeof(MfmGemmDesc) * cnt);
    for (int i = 0; i < cnt; ++i) fill(p0 + i, g[i]);
    const int rc = gemm_group_launch(g, cnt, stream);
    if (rc != MFM_OK) return rc;
  }
  return MFM_OK;
}

// the x-projection of LSTM s: gates [m, 4, Hp] = a [m, k] (rows lda apart) . W_ih[g h + u] + b_ih + b_hh; pad units u >= h exact zeros
static void xproj_desc(MfmGemmDesc& d, const SeqDev& s, const float* a, int64_t lda, int k, int m, float* gates) {
  d.a = a; d.a_sm = lda; d.a_sk = 1; d.a_sz = 0;
  d.b = s.w_ih; d.b_sz = (int64_t)s.h * k; d.b_sn = k; d.b_sk = 1;
  d.c = gates; d.c_sz = s.Hp; d.ldc = 4 * (int64_t)s.Hp;
  d.bias = s.b_ih; d.bias2 = s.b_hh; d.bias_sz = s.h;
  d.m = m; d.n = s.Hp; d.n_valid = s.h; d.k = k; d.batch = 4; d.split_k = 1;
  d.alpha = 1.0f;
}

// one LSTM of a call as the host walks it: where the caller's kernel argument keeps its SeqDev and (an MFN LSTM) its last hidden
// states -- the entries' *One structs differ --, and the d columns of x from col on that it projects
struct MfnLstm { SeqDev* seq; float** h_last; int col, d; };

// the x-projections of a chunk, rows [n0, n0 + n) of the split x [T, N, D], as ONE grouped GEMM: gates_e[t][i][g][u] =
// x_e[t][n0 + i] . W_ih[g h + u] + b_ih + b_hh, pad units u >= h exact zeros.  One chunk: the T * N rows of x are one matrix and
// an LSTM one problem; else one problem per LSTM and step
static int mfn_xproj_chunk(int count, const MfnLstm* L, const float* x, int T, int64_t N, int D, int64_t n0, int n, hipStream_t stream) {
  const bool whole = n == N;
  return gemm_group_each(count * (whole ? 1 : T), stream, [&](int p, MfmGemmDesc& d) {
    const int e = p % count, t = p / count;
    const SeqDev& s = *L[e].seq;
    xproj_desc(d, s, x + ((int64_t)t * N + n0) * D + L[e].col, D, L[e].d, whole ? T * n : n, s.gates + (int64_t)t * n * 4 * s.Hp);
  });
}

// fc1 of decoder s over its stored h: c [m, dm] = hs [m, Hp] . w^T + b, `batch` times a_sz / c_sz apart
static void dec_fc1_desc(MfmGemmDesc& d, const SeqDev& s, const float* hs, const float* w, const float* b, float* c, int dm, int m,
                         int batch = 1, int64_t a_sz = 0, int64_t c_sz = 0) {
  d.a = hs; d.a_sm = s.Hp; d.a_sk = 1; d.a_sz = a_sz;
  d.b = w; d.b_sn = s.h; d.b_sk = 1;
  d.c = c; d.ldc = dm; d.c_sz = c_sz;
  d.bias = b;
  d.m = m; d.n = dm; d.n_valid = dm; d.k = s.h; d.batch = batch; d.split_k = 1;
  d.alpha = 1.0f;
}

// ---------------------------------------------------------------- host: the two launch rules
// the kernel instantiated for s.hk4 alone: pick(std::integral_constant<int, hk4>) names it
template <class Dev, class Pick>
static int infer_launch_hk4(const char* who, const char* name, const SeqDev& s, Pick pick, const Dev& P, int grid, int threads,
                            size_t lds_bytes, hipStream_t stream) {
#define MFM_INFER_CASE(KK, ...) \
  case KK: return seq_launch_kernel(pick(std::integral_constant<int, KK>()), name, dim3(grid), dim3(threads), lds_bytes, stream, nullptr, P);
  switch (s.hk4) { MFM_HK4_CASES(MFM_INFER_CASE) }
#undef MFM_INFER_CASE
  set_error("%s: no kernel for h = %d", who, s.h);
  return MFM_ERR_UNSUPPORTED;
}

// the launch(es) of one chunk of P.n rows in tiles of R: the LSTMs P.d[0 .. P.count) in one launch of `canon`, the kernel of
// their canonical size tuple -- or, canon null (other sizes), one launch per LSTM of the kernel pick names for its size
template <int R, class Dev, class Pick>
static int infer_launch_tuple_or_each(const char* who, const char* name, Dev& P, void (*canon)(const Dev), Pick pick, int threads,
                                      size_t lds_bytes, hipStream_t stream) {
  const int tiles = cdiv(P.n, R);
  if (canon) {
    for (int i = 0; i < P.count; ++i) P.d[i].block_begin = i * tiles;
    return seq_launch_kernel(canon, name, dim3(P.count * tiles), dim3(threads), lds_bytes, stream, nullptr, P);
  }
  for (int i = 0; i < P.count; ++i) {
    Dev Q = P;
    Q.d[0] = P.d[i]; Q.d[0].block_begin = 0; Q.count = 1;
    const int rc = infer_launch_hk4(who, name, Q.d[0].seq, pick, Q, tiles, std::max(8 * Q.d[0].seq.Hp, 64), lds_bytes, stream);
    if (rc != MFM_OK) return rc;
  }
  return MFM_OK;
}

}  // namespace mfm
