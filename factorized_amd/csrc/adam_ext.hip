// Fused Adam / AdamW / AMSGrad over spans of one flat parameter buffer, every span with its own hyper-parameters and step count
// (torch.optim.Adam semantics, _single_tensor_adam's non-capturable branch; factorized_amd.optim.Adam / AdamW).
//
// Traffic per element of a span: p, m, v read and written, g read = 28 B; a span with MFM_ADAMX_AMSGRAD also reads and writes
// vmax = 36 B.  A span without the flag neither reads nor writes vmax.
#include "adam_dev.h"
#include "span_tiles.h"

namespace mfm {

// One span in kernel form: the common head, the coefficients of its hyper-parameters and step count (adam_coef, as adam_launch
// forms them) and its weight decay.
// `decay` is weight_decay for L2 decay (g += decay * p) and 1 - lr * weight_decay for decoupled decay (p *= decay).
struct AdamxSpanDev {
  SpanHead h;
  AdamCoef c;
  float decay;
};
// 88 x 40 bytes + 8 = 3528: well inside the 4 KiB a kernel argument block may hold
struct AdamxSpansDev {
  AdamxSpanDev s[MFM_ADAMX_MAX_SPANS];
  int32_t count, tiles;
};
static_assert(sizeof(AdamxSpansDev) + 6 * sizeof(void*) + 8 <= 4096, "Adam span table exceeds the kernel argument limit");

constexpr int kAdamxDecay = 1 << 30;  // (device table only) the span has weight_decay != 0

// Work is dealt in tiles as span_tiles.h describes.  The update is adam_kernel's (adam_dev.h), the options its uniform
// arguments: a span with no option set executes what adam_kernel executes.
__global__ __launch_bounds__(kSpanTile) void adam_ext_spans_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                   float* __restrict__ m, float* __restrict__ v,
                                                                   float* __restrict__ vmax, const AdamxSpansDev S,
                                                                   float grad_scale, const float* __restrict__ guard) {
  // guard word (mfm_adam_ext_flat_spans_guarded): raised, it leaves p, m, v and vmax as they are
  if (guard_raised(guard)) return;
  int k = 0;
  for (int t = blockIdx.x; t < S.tiles; t += gridDim.x) {
    k = span_of_tile(S, t, k);
    const AdamxSpanDev sp = S.s[k];
    const int64_t i = span_tile_index(sp.h, t);
    if (i >= sp.h.e4) continue;
    const bool amsgrad = (sp.h.flags & MFM_ADAMX_AMSGRAD) != 0;
    const bool decay = (sp.h.flags & kAdamxDecay) != 0;
    const bool decoupled = (sp.h.flags & MFM_ADAMX_DECOUPLED) != 0;
    const float gs = (sp.h.flags & MFM_ADAMX_MAXIMIZE) ? -grad_scale : grad_scale;
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    f32x4 mv = reinterpret_cast<f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
    f32x4 xv = {0.0f, 0.0f, 0.0f, 0.0f};
    if (amsgrad) xv = reinterpret_cast<const f32x4*>(vmax)[i];
    if (decay && decoupled) pv = pv * sp.decay;      // param.mul_(1 - lr * weight_decay)
    adam_update4(pv, mv, vv, gv, sp.c, gs, decay && !decoupled, sp.decay, amsgrad, &xv);
    reinterpret_cast<f32x4*>(p)[i] = pv;
    reinterpret_cast<f32x4*>(m)[i] = mv;
    reinterpret_cast<f32x4*>(v)[i] = vv;
    if (amsgrad) reinterpret_cast<f32x4*>(vmax)[i] = xv;
  }
}

int adam_ext_spans_launch(float* p, const float* g, float* m, float* v, float* vmax, const MfmAdamExtSpan* spans, int nspans,
                          float grad_scale, hipStream_t stream, const float* guard) {
  MFM_REQUIRE(p && g && m && v && spans && nspans >= 1 && nspans <= MFM_ADAMX_MAX_SPANS,
              "adam ext spans: bad arguments (nspans=%d, at most %d)", nspans, MFM_ADAMX_MAX_SPANS);
  MFM_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vmax) & 15) == 0,
              "adam ext spans: buffers must be 16-byte aligned");
  AdamxSpansDev S;
  memset(&S, 0, sizeof(S));
  S.count = nspans;
  int64_t tiles = 0, prev_end = 0;
  for (int k = 0; k < nspans; ++k) {
    const MfmAdamExtSpan& sp = spans[k];
    AdamxSpanDev& d = S.s[k];
    if (int rc = span_head_fill("adam ext spans", k, sp.begin, sp.end, &prev_end, &tiles, &d.h)) return rc;
    MFM_REQUIRE(sp.step >= 1, "adam ext spans[%d]: step %d (1-based, must be >= 1)", k, sp.step);
    MFM_REQUIRE(sp.lr >= 0.0f && sp.eps >= 0.0f && sp.weight_decay >= 0.0f,
                "adam ext spans[%d]: lr %g, eps %g, weight_decay %g (each must be >= 0)", k, (double)sp.lr, (double)sp.eps,
                (double)sp.weight_decay);
    MFM_REQUIRE(sp.beta1 >= 0.0f && sp.beta1 < 1.0f && sp.beta2 >= 0.0f && sp.beta2 < 1.0f,
                "adam ext spans[%d]: beta1 %g, beta2 %g (each must be in [0, 1))", k, (double)sp.beta1, (double)sp.beta2);
    MFM_REQUIRE((sp.flags & ~(MFM_ADAMX_MAXIMIZE | MFM_ADAMX_AMSGRAD | MFM_ADAMX_DECOUPLED)) == 0,
                "adam ext spans[%d]: unknown flags 0x%x", k, (unsigned)sp.flags);
    MFM_REQUIRE(vmax || !(sp.flags & MFM_ADAMX_AMSGRAD), "adam ext spans[%d]: AMSGRAD needs a vmax buffer", k);
    d.h.flags = sp.flags | (sp.weight_decay != 0.0f ? kAdamxDecay : 0);
    d.c = adam_coef(sp.lr, sp.beta1, sp.beta2, sp.eps, sp.step);
    d.decay = (sp.flags & MFM_ADAMX_DECOUPLED) ? (float)(1.0 - (double)sp.lr * (double)sp.weight_decay) : sp.weight_decay;
  }
  int nb;
  if (int rc = span_grid("adam ext spans", tiles, &S.tiles, &nb)) return rc;
  MFM_LAUNCH_TIMED(adam_ext_spans_kernel, dim3(nb), dim3(kSpanTile), 0, stream, p, g, m, v, vmax, S, grad_scale, guard);
  MFM_LAUNCH_CHECK("adam_ext_spans_kernel");
  return MFM_OK;
}

}  // namespace mfm

extern "C" int mfm_adam_ext_flat_spans(float* p, const float* g, float* m, float* v, float* vmax, const MfmAdamExtSpan* spans,
                                       int32_t nspans, float grad_scale, void* stream) {
  return mfm::adam_ext_spans_launch(p, g, m, v, vmax, spans, nspans, grad_scale, (hipStream_t)stream, nullptr);
}

extern "C" int mfm_adam_ext_flat_spans_guarded(float* p, const float* g, float* m, float* v, float* vmax,
                                               const MfmAdamExtSpan* spans, int32_t nspans, float grad_scale, const float* guard,
                                               void* stream) {
  return mfm::adam_ext_spans_launch(p, g, m, v, vmax, spans, nspans, grad_scale, (hipStream_t)stream, guard);
}
