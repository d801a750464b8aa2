// The encoder half of MFM_KL and MFM (include/mfm_hip.h, mfm_encode_mfn): the three modality encoders and the Memory Fusion
// Network behind the label factor (mfm_model.py:140-199, :723-743) as one call -- no plan, no training workspace, in the
// pattern of mfm_encode_klef (generate.hip, infer_dev.h).  Per row chunk:
//   1. the six input projections (encoder l, a, v and the MFN's LSTM l, a, v on their column ranges of x) as ONE grouped fp32
//      GEMM (a chunk that is not the whole split: one problem per LSTM and time step);
//   2. encode_mfn_seq_kernel: workgroup (LSTM, row tile) runs the T-step recurrence on chip.  An encoder goes on with its fc1
//      (and, with heads, the mean and logvar heads) on the last hidden states still in LDS; an MFN LSTM stores its cell states
//      c_t (small_fwd_body's CS mode: no h record, no gates) and its last hidden state;
//   3. encode_mfn_att_kernel: row-wise over the T * n pairs (t, i).  A workgroup gathers cStar = [c_{t-1} | c_t] of 16 or 32
//      pairs into LDS as [k][pair] and runs att1_fc1 -> relu -> att1_fc2 -> softmax -> * cStar -> att2_fc1 -> relu -> att2_fc2 ->
//      tanh and the attended columns of gamma1_fc1 / gamma2_fc1 on v_mfma_f32_16x16x4_f32: the pairs are the N dimension, 16
//      output units the M dimension, the weights stream from L2 as the A operand (16 bytes per lane and 16 k).  cStar,
//      attention and attended never leave LDS; per pair cHat and the two partial gamma pre-activations are written;
//   4. encode_mfn_mem_kernel: one workgroup per row runs the T steps of the memory with the four small matrices (the memory
//      columns of gamma*_fc1, gamma*_fc2) in registers and mem / the relu activations in LDS -- the forward of mfn_mem.hip without
//      its records -- and ends with last_to_zy_fc1 (and the logvar head) on [h_l | h_a | h_v | mem].
// A pair's and a row's arithmetic does not depend on its place in a tile or a chunk, nothing is accumulated across workgroups:
// results are bit-identical from run to run, and for every chunking within one tile-row form of launch 2 (gen_tile_rows).
// The kernels and the host side every MFN entry shares live in encode_mfn_dev.h (its file head lists them); the walk over the four
// launches (emfn_front_prepare / emfn_front_chunk) in encode_mfn_front.h, which mfm_objective_mfn (objective_mfn.hip) runs too.
#include "encode_mfn_front.h"

namespace mfm {

static int encode_mfn(int T, int64_t N, const int32_t* sz, const float* params, const int64_t* offs, const float* x, float* ws,
                      float* const* out, int64_t max_rows, hipStream_t stream) {
  static const char* who = "encode mfn";
  EmfnSizes S;
  MFM_REQUIRE(T >= 1 && N >= 1 && emfn_sizes(sz, S), "%s: sizes must be positive (T %d, N %lld, and the %d sizes; the last 0 or 1)", who, T,
              (long long)N, EMFN_SIZES);
  MFM_REQUIRE(params && offs && x && ws && out, "%s: bad arguments (params, offsets, x, workspace and outputs must not be null)", who);
  for (int i = 0; i < (S.heads ? 8 : 4); ++i) MFM_REQUIRE(out[i], "%s: output %d is null", who, i);
  int rc = infer_check_aligned(who, params, x, ws);
  if (rc != MFM_OK) return rc;
  EmfnWs W;
  emfn_ws(S, T, gen_rows(N, max_rows), W);
  EmfnFront F;
  if ((rc = emfn_front_prepare(who, T, N, S, params, offs, ws, ws + W.all_gates, max_rows, F)) != MFM_OK) return rc;
  for (int64_t n0 = 0; n0 < N; n0 += F.rows) {
    const int n = (int)std::min<int64_t>(F.rows, N - n0);
    float* oc[8];
    for (int i = 0; i < 8; ++i) oc[i] = (i < 4 || S.heads) ? out[i] + n0 * (i % 4 < 3 ? S.z[i % 4] : S.zy) : nullptr;
    if ((rc = emfn_front_chunk(who, F, x, N, n0, n, oc, stream)) != MFM_OK) return rc;
  }
  return MFM_OK;
}

}  // namespace mfm

extern "C" int64_t mfm_encode_mfn_workspace_floats(int32_t T, int64_t N, const int32_t* sizes, int64_t max_rows) {
  mfm::EmfnSizes S;
  if (T < 1 || N < 1 || max_rows < 0 || !mfm::emfn_sizes(sizes, S)) return 0;
  mfm::EmfnWs W;
  mfm::emfn_ws(S, T, mfm::gen_rows(N, max_rows), W);
  return W.total;
}

extern "C" int mfm_encode_mfn_tile_rows(int64_t N, int64_t max_rows) {
  if (N < 1 || max_rows < 0) return -1;
  return mfm::gen_tile_rows(EMFN_LSTMS, (int)mfm::gen_rows(N, max_rows));
}

extern "C" int mfm_encode_mfn(int32_t T, int64_t N, const int32_t* sizes, const float* params, const int64_t* offsets, const float* x,
                              float* workspace, float* const* out, int64_t max_rows, void* stream) {
  return mfm::encode_mfn(T, N, sizes, params, offsets, x, workspace, out, max_rows, (hipStream_t)stream);
}
