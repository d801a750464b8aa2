// Fused momentum SGD over spans of one flat parameter buffer (torch.optim.SGD semantics; factorized_amd.optim.SGD).
#include "span_tiles.h"

namespace mfm {

// One span in kernel form: the common head and the hyper-parameters the update needs (1 - dampening formed on the host in
// double precision, as torch's Python scalar is).
struct SgdSpanDev {
  SpanHead h;
  float lr, wd, mom, omd;
};
// 112 x 32 bytes + 8: well inside the 4 KiB a kernel argument block may hold
struct SgdSpansDev {
  SgdSpanDev s[MFM_SGD_MAX_SPANS];
  int32_t count, tiles;
};
static_assert(sizeof(SgdSpansDev) + 4 * sizeof(void*) + 8 <= 4096, "SGD span table exceeds the kernel argument limit");

// Work is dealt in tiles as span_tiles.h describes.
__global__ __launch_bounds__(kSpanTile) void sgd_spans_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                              float* __restrict__ buf, const SgdSpansDev S, float grad_scale,
                                                              const float* __restrict__ guard) {
  // guard word (mfm_sgd_flat_spans_guarded): raised, it leaves p and buf as they are
  if (guard_raised(guard)) return;
  int k = 0;
  for (int t = blockIdx.x; t < S.tiles; t += gridDim.x) {
    k = span_of_tile(S, t, k);
    const SgdSpanDev sp = S.s[k];
    const int64_t i = span_tile_index(sp.h, t);
    if (i >= sp.h.e4) continue;
    const bool maximize = (sp.h.flags & MFM_SGD_MAXIMIZE) != 0;
    const float gs = maximize ? -grad_scale : grad_scale;
    f32x4 pv = reinterpret_cast<f32x4*>(p)[i];
    const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
    if (sp.mom != 0.0f) {
      const bool first = (sp.h.flags & MFM_SGD_FIRST) != 0;
      const bool nesterov = (sp.h.flags & MFM_SGD_NESTEROV) != 0;
      // a first step creates the buffer (torch: clone of the gradient): the old contents are not read
      f32x4 bv = first ? f32x4{0.0f, 0.0f, 0.0f, 0.0f} : reinterpret_cast<const f32x4*>(buf)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float d = gv[j] * gs;
        if (sp.wd != 0.0f) d = fmaf(sp.wd, pv[j], d);                 // grad.add(param, alpha=weight_decay)
        const float b = first ? d : fmaf(sp.omd, d, bv[j] * sp.mom);    // buf.mul_(momentum).add_(grad, alpha=1-dampening)
        d = nesterov ? fmaf(sp.mom, b, d) : b;
        pv[j] = fmaf(-sp.lr, d, pv[j]);                                 // param.add_(grad, alpha=-lr)
        bv[j] = b;
      }
      reinterpret_cast<f32x4*>(buf)[i] = bv;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float d = gv[j] * gs;
        if (sp.wd != 0.0f) d = fmaf(sp.wd, pv[j], d);
        pv[j] = fmaf(-sp.lr, d, pv[j]);
      }
    }
    reinterpret_cast<f32x4*>(p)[i] = pv;
  }
}

int sgd_spans_launch(float* p, const float* g, float* buf, const MfmSgdSpan* spans, int nspans, float grad_scale,
                     hipStream_t stream, const float* guard) {
  MFM_REQUIRE(p && g && spans && nspans >= 1 && nspans <= MFM_SGD_MAX_SPANS, "sgd spans: bad arguments (nspans=%d, at most %d)",
              nspans, MFM_SGD_MAX_SPANS);
  MFM_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf) & 15) == 0, "sgd spans: buffers must be 16-byte aligned");
  SgdSpansDev S;
  memset(&S, 0, sizeof(S));
  S.count = nspans;
  int64_t tiles = 0, prev_end = 0;
  for (int k = 0; k < nspans; ++k) {
    const MfmSgdSpan& sp = spans[k];
    SgdSpanDev& d = S.s[k];
    if (int rc = span_head_fill("sgd spans", k, sp.begin, sp.end, &prev_end, &tiles, &d.h)) return rc;
    MFM_REQUIRE(sp.lr >= 0.0f && sp.weight_decay >= 0.0f && sp.momentum >= 0.0f,
                "sgd spans[%d]: lr %g, weight_decay %g, momentum %g (each must be >= 0)", k, (double)sp.lr,
                (double)sp.weight_decay, (double)sp.momentum);
    MFM_REQUIRE((sp.flags & ~(MFM_SGD_NESTEROV | MFM_SGD_MAXIMIZE | MFM_SGD_FIRST)) == 0, "sgd spans[%d]: unknown flags 0x%x", k,
                (unsigned)sp.flags);
    MFM_REQUIRE(buf || sp.momentum == 0.0f, "sgd spans[%d]: momentum %g needs a momentum buffer", k, (double)sp.momentum);
    d.h.flags = sp.flags;
    d.lr = sp.lr;
    d.wd = sp.weight_decay;
    d.mom = sp.momentum;
    d.omd = (float)(1.0 - (double)sp.dampening);
  }
  int nb;
  if (int rc = span_grid("sgd spans", tiles, &S.tiles, &nb)) return rc;
  MFM_LAUNCH_TIMED(sgd_spans_kernel, dim3(nb), dim3(kSpanTile), 0, stream, p, g, buf, S, grad_scale, guard);
  MFM_LAUNCH_CHECK("sgd_spans_kernel");
  return MFM_OK;
}

}  // namespace mfm

extern "C" int mfm_sgd_flat_spans(float* p, const float* g, float* buf, const MfmSgdSpan* spans, int32_t nspans, float grad_scale,
                                  void* stream) {
  return mfm::sgd_spans_launch(p, g, buf, spans, nspans, grad_scale, (hipStream_t)stream, nullptr);
}

extern "C" int mfm_sgd_flat_spans_guarded(float* p, const float* g, float* buf, const MfmSgdSpan* spans, int32_t nspans,
                                          float grad_scale, const float* guard, void* stream) {
  return mfm::sgd_spans_launch(p, g, buf, spans, nspans, grad_scale, (hipStream_t)stream, guard);
}
