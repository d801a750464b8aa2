// Row-wise dense layer of the inference launches (predict.hip, generate.hip): the R batch rows of a workgroup's tile through one
// nn.Linear, activations in LDS, the weights straight from L2.
#pragma once
#include "lstm_seq_small_dev.h"

namespace mfm {

// out[c][r] = act(bias[c] + sum_k W[c][k] in[k][r]) for the tile's R rows; in / out are LDS, [.][R].  A quad of lanes per
// output column, lane q takes the 16-byte blocks k = 4 q + 16 j (K % 4 == 0 and an aligned row) or the elements k = q + 4 j.
template <int R>
__device__ __forceinline__ void dense_rows(const float* __restrict__ W, const float* __restrict__ bias, const int K, const int N,
                                           const float* in, float* out, const bool relu) {
  const int tid = threadIdx.x, nq = blockDim.x >> 2, q = tid & 3;
  const bool vec = (K & 3) == 0 && (((uintptr_t)W) & 15) == 0;
  for (int c = tid >> 2; c < N; c += nq) {
    const float* wr = W + (int64_t)c * K;
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0f;
    if (vec) {
      for (int k0 = 4 * q; k0 < K; k0 += 16) {
        const f32x4 w4 = *reinterpret_cast<const f32x4*>(wr + k0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const RowVec<R> xv = ld_rows<R>(in + (k0 + i) * R);
#pragma unroll
          for (int r = 0; r < R; ++r) acc[r] = fmaf(w4[i], xv.v[r], acc[r]);
        }
      }
    } else {
      for (int k = q; k < K; k += 4) {
        const float wv = wr[k];
        const RowVec<R> xv = ld_rows<R>(in + k * R);
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fmaf(wv, xv.v[r], acc[r]);
      }
    }
    const float bv = bias[c];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float v = acc[r];
      v += dpp_f<DPP_QUAD_XOR1>(v);
      v += dpp_f<DPP_QUAD_XOR2>(v);
      v += bv;
      if (relu) v = fmaxf(v, 0.0f);
      if (q == 0) out[c * R + r] = v;
    }
  }
  lds_barrier();
}

}  // namespace mfm
