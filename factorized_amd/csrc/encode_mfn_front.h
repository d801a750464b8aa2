// The encoder half of MFM_KL and MFM chunk by chunk, as mfm_encode_mfn (encode_mfn.hip) and mfm_objective_mfn (objective_mfn.hip)
// run it: the grouped projection GEMM, the six recurrences in one launch (emfn_seq_launch), the attention chain and the memory
// recurrence with the label head(s).  Everything but the launch of the six recurrences is the shared host side of
// encode_mfn_dev.h.  A header of its own: zeros_mfn.hip and predict_mfn.hip include encode_mfn_dev.h and must not instantiate
// encode_mfn_seq_kernel.
#pragma once
#include "encode_mfn_dev.h"

namespace mfm {

// prepare: the checks behind the caller's own argument checks (row cap, offsets, the refusals), then everything of the four
// launches that does not depend on the chunk.  gates: where the six x-projections of a chunk go (EmfnWs.all_gates floats in all); rest:
// the parts behind them (c records, last hidden states, cHat, the gamma partials), in the order of mfn_ws.
// chunk: the launches of one chunk of n <= rows rows.  L points into P: an EmfnFront stays where prepare filled it
struct EmfnFront {
  EmfnSizes S; EmfnSeqDev P; EmfnChain C; MfnLstm L[EMFN_LSTMS];
  int T, rows, R, threads, D, n_offs;
  size_t seq_lds;
};

static int emfn_front_prepare(const char* who, int T, int64_t N, const EmfnSizes& S, const float* params, const int64_t* offs, float* gates,
                              float* rest, int64_t max_rows, EmfnFront& F) {
  int rc = infer_check_rows(who, N, max_rows);
  if (rc != MFM_OK) return rc;
  const int EO = S.heads ? 10 : 6, o_mfn = 3 * EO, o_att = o_mfn + 12, o_zy = o_att + 16, n_offs = o_zy + (S.heads ? 4 : 2);
  if ((rc = infer_check_offsets(who, offs, o_mfn, EO)) != MFM_OK) return rc;
  if ((rc = infer_check_offsets(who, offs + o_mfn, n_offs - o_mfn, 4, 0, 12)) != MFM_OK) return rc;
  if ((rc = mfn_check_covered(who, S, true)) != MFM_OK) return rc;
  const int D = S.d[0] + S.d[1] + S.d[2];
  const int rows = (int)gen_rows(N, max_rows);
  const int R = gen_tile_rows(EMFN_LSTMS, rows);
  int maxw = 1, threads = 64;
  size_t seq_floats = 0;
  for (int i = 0; i < EMFN_LSTMS; ++i) {
    const int h = i < 3 ? S.z[i] : S.hm[i - 3];
    maxw = std::max(maxw, h);
    threads = std::max(threads, 8 * round_up(h, 16));
  }
  for (int i = 0; i < EMFN_LSTMS; ++i)
    seq_floats = std::max(seq_floats, i < 3 ? enc_lds_floats(S.z[i], R, 3, maxw) : seq_lds_floats(S.hm[i - 3], R));
  const size_t seq_lds = lds_bytes_of(seq_floats);
  if ((rc = infer_check_lds(who, seq_lds, maxw, R)) != MFM_OK) return rc;
  // the attention chain and the memory recurrence
  if ((rc = emfn_chain_check(who, S, (int64_t)T * rows, F.C)) != MFM_OK) return rc;
  if ((rc = infer_check_chunk(who, rows, T, std::max(std::max(D, 4 * round_up(maxw, 16)), std::max(S.M, std::max(S.H1, S.H2))), "projection")) != MFM_OK) return rc;

  // ---- everything that does not depend on the chunk
  EmfnSeqDev& P = F.P;
  F.S = S;
  EmfnWs W;
  emfn_ws(S, T, rows, W);
  memset(&P, 0, sizeof(P));
  float* w0 = gates;
  for (int i = 0; i < 3; ++i) {          // the encoders; the MFN's LSTMs behind them
    EmfnOne& E = P.d[i];
    const int64_t* o = offs + EO * i;
    seq_fill(E.seq, params + o[0], params + o[1], params + o[2], params + o[3], S.z[i], 0);
    E.seq.gates = w0; w0 += W.gates[i];
    for (int l = 0; l < (S.heads ? 3 : 1); ++l) { E.w[l] = params + o[4 + 2 * l]; E.b[l] = params + o[5 + 2 * l]; }
    F.L[i] = MfnLstm{&E.seq, nullptr, mfn_col(S, i), S.d[i]};
  }
  for (int m = 0; m < 3; ++m) F.L[3 + m] = MfnLstm{&P.d[3 + m].seq, &P.d[3 + m].h_last, 0, 0};
  mfn_lstms_fill(F.L + 3, F.C, S, T, rows, 1, params, offs + o_mfn, w0, rest);
  P.count = EMFN_LSTMS; P.T = T; P.maxw = maxw; P.heads = S.heads;
  emfn_chain_fill(F.C, S, T, params, offs + o_att, offs + o_zy, S.heads ? 2 : 1);
  F.T = T; F.rows = rows; F.R = R; F.threads = threads; F.D = D; F.n_offs = n_offs; F.seq_lds = seq_lds;
  return MFM_OK;
}

// x: the whole split [T, N, D], the chunk its rows [n0, n0 + n); out: the chunk's first rows of the four means, then (heads) the
// four log-variances
static int emfn_front_chunk(const char* who, EmfnFront& F, const float* x, int64_t N, int64_t n0, int n, float* const* out, hipStream_t stream) {
  EmfnSeqDev& P = F.P;
  const int T = F.T, D = F.D, heads = F.S.heads;
  int rc = mfn_xproj_chunk(EMFN_LSTMS, F.L, x, T, N, D, n0, n, stream);
  if (rc != MFM_OK) return rc;
  P.n = n;
  for (int i = 0; i < 3; ++i) { P.d[i].mu = out[i]; P.d[i].lv = heads ? out[4 + i] : nullptr; }
  rc = (F.R == 1) ? emfn_seq_launch<1>(who, P, F.threads, F.seq_lds, stream) : emfn_seq_launch<4>(who, P, F.threads, F.seq_lds, stream);
  if (rc != MFM_OK) return rc;
  F.C.Mm.oz[0] = out[3];
  F.C.Mm.oz[1] = heads ? out[7] : nullptr;
  return emfn_chain_launch<false>(F.C, T, n, stream);
}

}  // namespace mfm
