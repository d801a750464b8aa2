// Device-side descriptors shared by the two LSTM sequence kernel families.
#pragma once
#include "common.h"

namespace mfm {

struct SeqDev {
  float* gates; float* hs; float* cs;
  const float* w_hh; const float* w_ih; const float* b_ih; const float* b_hh;
  const float* h_init; int64_t ld_init;
  const float* dh_ext; int64_t ld_dh;
  float* d_h_init; int64_t ld_dinit;
  const float* dc_ext;
  const void* w_pack;      // bf16 path: packed weight fragments (mfm_lstm_pack_bf16), or null
  float* h_last;           // bf16 path, optional: fp32 copy of h_{T-1} [B, Hp]
  int h, Hp, hk4, is_dec, block_begin;
  int store_bf16;          // bf16 path: gates / hs / the decoders' dh_ext are __bf16 buffers (MfmSeqDesc::store_bf16)
  const float* wt_img;     // fp32 one-row BPTT, optional: this step's transposed weights in thread order (proj_role_dev.h), or null
  const float* wf_img;     // fp32 one-row forward, decoders, optional: W_ih + W_hh of this step in the forward's thread order, or null
  const float* wf1_img;    // the same for W_ih alone (the decoders' step 0), or null
};
// Transposed-weight images for the one-row BPTT kernels of the same step (lstm_seq_small.hip, small_bwd_body<.., KS = 16>):
// img4[s / 4][tid][s % 4], s = which * 4 NG + g * NG + i, holds W[g h + 16 i + (tid & 15)][2 (tid >> 4) + which] (w_ih set: W_ih + W_hh,
// the decoders' steps >= 1), zero outside the valid units.  Written by workgroups that have nothing else to do in a FORWARD
// launch of the step -- the projection role workgroups once their items are done (proj_role_dev.h), or a few blocks appended to
// the recurrence launch -- and read by the BPTT launches, which come later in the stream: nothing has to be signalled.
struct WtImgItem { const float* w_hh; const float* w_ih; float* img; int h, HKB; int fwd; };     // fwd: a forward-order image (below)
constexpr int MFM_WT_MAX = MFM_MAX_SEQ + 3;
constexpr int MFM_IMG_MAX = MFM_WT_MAX + 6;      // + the decoders' forward-order images (W_ih, W_ih + W_hh)
struct SeqLaunch {
  SeqDev d[MFM_MAX_SEQ];
  int count, T, B;
  // forward launches, optional: blocks [img_begin, img_begin + n_img_blocks) write the images of `img` and leave
  int n_img, img_begin, n_img_blocks;
  WtImgItem img[MFM_IMG_MAX];
  int bf16_dot;            // one-row forward kernels: recurrent product on bf16 dot products (MfmSeqDesc::bf16_dot on every LSTM)
};

__device__ __forceinline__ void wf_img_write(const WtImgItem* items, const int n, const int r, const int nr);
// writer r of nr (any block size); items marked `fwd` are written in the forward's register order (wf_img_write)
__device__ __forceinline__ void wt_img_write(const WtImgItem* items, const int n, const int r, const int nr) {
  const int tid = threadIdx.x, nt = blockDim.x;
#pragma unroll 1
  for (int w = 0; w < n; ++w) {
    const WtImgItem& I = items[w];
    if (I.fwd) { wf_img_write(&I, 1, r, nr); continue; }
    // (round 6: four consecutive slots of a thread side by side -- img4[(s / 4) NTH + tid][s % 4] -- so that the BPTT takes its
    // 2 NW registers with NW / 2 16-byte loads instead of 2 NW 4-byte ones; 4 NG slots per `which`: a quad never straddles it)
    const int NG = I.HKB >> 4, NTH = 8 * I.HKB, h = I.h;
    const int total = 2 * NG * NTH;
    f32x4* out = reinterpret_cast<f32x4*>(I.img);
    // 64-quad pieces (one wave, 1 KB) dealt round-robin over the WRITERS first, then over a writer's waves: the largest image
    // is 256 pieces, and dealt thread by thread they all landed on the first 16 of 128 role workgroups
    const int nwv = nt >> 6;
    for (int c = (tid >> 6) * nr + r; c * 64 < total; c += nwv * nr) {
      const int idx = c * 64 + (tid & 63);
      if (idx >= total) break;
      const int s4 = idx / NTH, t2 = idx - s4 * NTH;
      f32x4 v4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int s = 4 * s4 + e;
        const int which = s / (4 * NG), rem = s - which * 4 * NG;
        const int g = rem / NG, i = rem - g * NG;
        const int j = 16 * i + (t2 & 15), u = 2 * (t2 >> 4) + which;
        float v = 0.0f;
        if (j < h && u < h) {
          v = I.w_hh[((int64_t)g * h + j) * h + u];
          if (I.w_ih) v += I.w_ih[((int64_t)g * h + j) * h + u];
        }
        v4[e] = v;
      }
      out[idx] = v4;
    }
  }
}

// Forward-order image of a decoder's steps >= 1 weights (round 6; the launch clock, profiles/r06_launch_timeline.txt, put the
// decoders' mid-launch reload of W_ih + W_hh at 6.4 us: two strided 16-byte gathers per register quad and an add, behind step
// 0): img4[(gl * NM + m) * NTH + tid] = (W_ih + W_hh)[(2 gp + gl) h + u][16 m + 4 q .. + 3] with q = tid & 3, gp = (tid >> 2) & 1,
// u = tid >> 3, NM = HKB / 16, NTH = 8 HKB -- exactly the registers w[gl][4 m ..] of small_fwd_body<KQ, 1>, so the reload is 2 NM
// coalesced 16-byte loads per thread.  Zero outside the valid units.  Written like the transposed images (role workgroups of
// the encoder launch), read by the decoder launch behind it.  h % 4 == 0 only.  An item without w_hh: the image of W_ih alone
// (step 0: 3.0 -> 1.5 us for h = 104, the same strided gather without the add).
__device__ __forceinline__ void wf_img_write(const WtImgItem* items, const int n, const int r, const int nr) {
  const int tid = threadIdx.x, nt = blockDim.x;
#pragma unroll 1
  for (int w = 0; w < n; ++w) {
    const WtImgItem& I = items[w];
    const int NM = I.HKB >> 4, NTH = 8 * I.HKB, h = I.h;
    const int total = 2 * NM * NTH;
    f32x4* out = reinterpret_cast<f32x4*>(I.img);
    for (int idx = r * nt + tid; idx < total; idx += nr * nt) {
      const int s = idx / NTH, t2 = idx - s * NTH;
      const int gl = s / NM, m = s - gl * NM;
      const int q = t2 & 3, gp = (t2 >> 2) & 1, u = t2 >> 3;
      const int k0 = 16 * m + 4 * q;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (u < h && k0 < h) {
        const int64_t o = ((int64_t)(2 * gp + gl) * h + u) * h + k0;
        v = *reinterpret_cast<const f32x4*>(I.w_ih + o);
        if (I.w_hh) v = *reinterpret_cast<const f32x4*>(I.w_hh + o) + v;
      }
      out[idx] = v;
    }
  }
}

// ---------------------------------------------------------------- kernel wrappers: what every sequence kernel opens with
// declares `di`: the LSTM that block `bid` of the multi-LSTM launch L belongs to (its tile: bid - L.d[di].block_begin).  A macro:
// as an inlined function the same loop comes out with other scalar registers, and these kernels are kept instruction for instruction
// (any launch descriptor with `count` and a per-LSTM array `d` whose elements carry block_begin: SeqLaunch, those of infer_dev.h)
#define MFM_SEQ_BLOCK_LSTM(L, bid, di) \
  int di = 0;                          \
  _Pragma("unroll 1")                  \
  for (int i = 1; i < (L).count; ++i)  \
    if ((bid) >= (L).d[i].block_begin) di = i;
// every SeqDev::hk4 the weight-resident kernels are instantiated for: X(hk4, ...) once per value
#define MFM_HK4_CASES(X, ...)                                                                                         \
  X(2, __VA_ARGS__) X(4, __VA_ARGS__) X(6, __VA_ARGS__) X(8, __VA_ARGS__) X(10, __VA_ARGS__) X(12, __VA_ARGS__)      \
  X(14, __VA_ARGS__) X(16, __VA_ARGS__) X(18, __VA_ARGS__) X(20, __VA_ARGS__) X(22, __VA_ARGS__) X(24, __VA_ARGS__)  \
  X(26, __VA_ARGS__) X(28, __VA_ARGS__) X(30, __VA_ARGS__) X(32, __VA_ARGS__)
// kernels instantiated for a size tuple <K0, K1, ...> (0: no such LSTM): the statement(s) given run for the LSTM `di` of this
// block, with KQ its hk4 as a constant
#define MFM_TUPLE_ONE(IDX, KK, ...) \
  if (KK > 0 && di == IDX) { constexpr int KQ = KK > 0 ? KK : 2; __VA_ARGS__; }
#define MFM_TUPLE3(...) MFM_TUPLE_ONE(0, K0, __VA_ARGS__) MFM_TUPLE_ONE(1, K1, __VA_ARGS__) MFM_TUPLE_ONE(2, K2, __VA_ARGS__)
#define MFM_TUPLE4(...) MFM_TUPLE3(__VA_ARGS__) MFM_TUPLE_ONE(3, K3, __VA_ARGS__)
#define MFM_TUPLE6(...) MFM_TUPLE4(__VA_ARGS__) MFM_TUPLE_ONE(4, K4, __VA_ARGS__) MFM_TUPLE_ONE(5, K5, __VA_ARGS__)

// ---------------------------------------------------------------- host: launching
// MFM_SEQ_KS / MFM_SEQ_ROWS are set: tuning overrides keep the plain launches
static inline bool seq_tuning_overrides() { return opt_get("MFM_SEQ_KS") != nullptr || opt_get("MFM_SEQ_ROWS") != nullptr; }

// One launch with `lds_bytes` of dynamic LDS: beyond the 64 KB a kernel may use unasked, its attribute is raised first -- to
// lds_bytes on every such launch, or with `once` (one flag per kernel) to all 160 KB the first time only: the attribute call
// is not a stream operation.  `name` is what an error is reported under; timed regions as MFM_LAUNCH_TIMED.
template <typename... KArgs, typename... Args>
static int seq_launch_kernel(void (*kernel)(KArgs...), const char* name, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream,
                             bool* once, const Args&... args) {
  if (lds_bytes > 64 * 1024 && !(once && *once)) {
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, once ? 160 * 1024 : (int)lds_bytes);
    if (e != hipSuccess) { char what[96]; snprintf(what, sizeof(what), "hipFuncSetAttribute(%s)", name); return hip_fail(e, what); }
    if (once) *once = true;
  }
  MFM_LAUNCH_TIMED(kernel, grid, block, lds_bytes, stream, args...);
  MFM_LAUNCH_CHECK(name);
  return MFM_OK;
}

// ---------------------------------------------------------------- host: the sequence launchers and what the plan asks them ahead of time
struct LatentDev;
struct ProjRole;
struct DwRole;
constexpr int MFM_SEQ_MAX_RESIDENT_H = 128;      // wider LSTMs take the step-by-step path
// lstm_seq.hip -- the entry points of the plan: descriptors in, one launch form each (SeqForm); MFM_ERR_UNSUPPORTED: not a case
// the form takes, nothing was launched
// encoder recurrences + their rows' latent chains (forward: optional image-writer blocks; backward: optional transposed images)
int seq_fold_launch(const MfmSeqDesc* descs, int count, int T, int B, bool bwd, const LatentDev& lat, const float* params,
                    float* grads, hipStream_t stream, const float* const* wt_imgs = nullptr, const WtImgItem* img_items = nullptr,
                    int n_img_items = 0, bool* img_written = nullptr);
// the forward fold launch with projection role workgroups in front (proj_role_dev.h)
int seq_foldproj_launch(const MfmSeqDesc* descs, int count, int T, int B, const LatentDev& lat, const float* params, ProjRole& pr,
                        hipStream_t stream);
// the backward fold launch with weight-gradient role workgroups behind the BPTT workgroups (dw_role_dev.h)
int seq_folddw_launch(const MfmSeqDesc* descs, int count, int T, int B, const LatentDev& lat, const float* params, float* grads,
                      DwRole& dr, hipStream_t stream, const float* const* wt_imgs = nullptr);
// plain forward launch with a few blocks behind the rows that write this step's weight images; *written: whether they did
int seq_fwd_img_launch(const MfmSeqDesc* descs, int count, int T, int B, const WtImgItem* items, int n_items, bool* written,
                       hipStream_t stream);
// plain BPTT launch whose one-row workgroups take their transposed weights from this step's images
int seq_bwd_img_launch(const MfmSeqDesc* descs, int count, int T, int B, const float* const* wt_imgs, hipStream_t stream);
// plain forward launch whose one-row decoder workgroups take their weights from this step's forward images: wf_imgs[0 .. count)
// W_ih + W_hh, wf_imgs[count .. 2 count) W_ih
int seq_fwd_wf_launch(const MfmSeqDesc* descs, int count, int T, int B, const float* const* wf_imgs, hipStream_t stream);
// decoder recurrences + the tail blocks of the latent forward chains
int seq_dec_tail_launch(const MfmSeqDesc* descs, int count, int T, int B, const float* const* wf_imgs, const LatentDev& lat,
                        const float* params, hipStream_t stream);
// decoder BPTTs + the head blocks of the latent backward chains
int seq_dec_bwd_head_launch(const MfmSeqDesc* descs, int count, int T, int B, const float* const* wt_imgs, const LatentDev& lat,
                            const float* params, float* grads, hipStream_t stream);
bool bf16_seq_pays(int B);     // batch size from which a bf16 plan runs its recurrences on the bf16 kernels
bool seq_mfma_pays(int B);     // batch size from which the fp32 resident recurrences run on the MFMA kernels (pick path)
// lstm_seq_small.hip -- fp32 VALU kernels, 1 / 4 rows per workgroup; L as filled by seq_launch, block layout by the launcher
int seq_small_launch(SeqLaunch& L, bool bwd, hipStream_t stream);      // the plain launch (+ image-writer blocks when L.n_img)
int seq_small_fold_launch(SeqLaunch& L, bool bwd, const LatentDev& LD, const float* params, float* grads, hipStream_t stream);
bool seq_small_foldproj_supported(int T, int B, const int* h, const int* k, int n_enc);     // shapes the projection roles take, idle CUs
int seq_small_foldproj_launch(SeqLaunch& L, const LatentDev& LD, ProjRole& PR, const float* params, hipStream_t stream);
bool seq_small_folddw_supported(int T, int B);      // room for the weight-gradient role workgroups behind 4 B rows
int seq_small_folddw_launch(SeqLaunch& L, const LatentDev& LD, DwRole& DR, const float* params, float* grads, hipStream_t stream);
bool seq_small_dectail_supported(int T, int B, const int* dec_h, const LatentDev& LD);      // can the decoder launch carry tail / head blocks?
int seq_small_dectail_launch(SeqLaunch& L, const LatentDev& LD, const float* params, hipStream_t stream);
int seq_small_decbwd_head_launch(SeqLaunch& L, const LatentDev& LD, const float* params, float* grads, hipStream_t stream);
// lstm_seq_bf16.hip: bf16 MFMA operands, fp32 accumulate / cell state / saved activations
int seq_bf16_launch(SeqLaunch& L, bool bwd, hipStream_t stream);
// lstm_step.hip: step-by-step path (recurrent GEMM + cell kernel per time step) for h > MFM_SEQ_MAX_RESIDENT_H
int seq_stepwise(const MfmSeqDesc* descs, int count, int T, int B, bool bwd, hipStream_t stream);

}  // namespace mfm
