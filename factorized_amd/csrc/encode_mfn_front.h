// The encoder half of MFM_KL and MFM chunk by chunk, as mfm_encode_mfn (encode_mfn.hip) and mfm_objective_mfn (objective_mfn.hip)
// run it: the grouped projection GEMM, the six recurrences in one launch, the attention chain and the memory recurrence with
// the label head(s) (encode_mfn_dev.h, ZC = false).  A header of its own: zeros_mfn.hip includes encode_mfn_dev.h for the chain
// on another gather and must not instantiate these launches.
#pragma once
#include "encode_mfn_dev.h"

namespace mfm {

// prepare: the checks behind the caller's own argument checks (row cap, offsets, the refusals), then everything of the four
// launches that does not depend on the chunk.  gates: where the six x-projections of a chunk go (W.gates floats in all); rest:
// the parts behind them (c records, last hidden states, cHat, the gamma partials), in the order of EmfnWs.
// chunk: the launches of one chunk of n <= rows rows
struct EmfnFront {
  EmfnSizes S; EmfnSeqDev P; EmfnChain C; EmfnWs W;
  int T, rows, R, threads, D, col[EMFN_LSTMS], dd[EMFN_LSTMS], n_offs;
  size_t seq_lds;
};

static int emfn_front_prepare(const char* who, int T, int64_t N, const EmfnSizes& S, const float* params, const int64_t* offs, float* gates,
                              float* rest, int64_t max_rows, EmfnFront& F) {
  int rc = infer_check_rows(who, N, max_rows);
  if (rc != MFM_OK) return rc;
  const int EO = S.heads ? 10 : 6, o_mfn = 3 * EO, o_att = o_mfn + 12, o_zy = o_att + 16, n_offs = o_zy + (S.heads ? 4 : 2);
  if ((rc = infer_check_offsets(who, offs, o_mfn, EO)) != MFM_OK) return rc;
  if ((rc = infer_check_offsets(who, offs + o_mfn, n_offs - o_mfn, 4, 0, 12)) != MFM_OK) return rc;

  // ---- what the kernels do not cover
  if (S.win != 2) {
    set_error("%s: windowsize %d (the attention reads the cell states of exactly 2 steps)", who, S.win);
    return MFM_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < 3; ++i) {
    if ((rc = infer_check_resident(who, S.z[i])) != MFM_OK) return rc;
    if ((rc = infer_check_resident(who, S.hm[i])) != MFM_OK) return rc;
  }
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
  EmfnAttDev& A = F.C.A;
  EmfnMemDev& Mm = F.C.Mm;
  EmfnSeqDev& P = F.P;
  F.S = S;
  emfn_ws(S, T, rows, F.W);
  memset(&P, 0, sizeof(P));
  float* w0 = gates;
  for (int i = 0; i < EMFN_LSTMS; ++i) {
    EmfnOne& E = P.d[i];
    const int m = i % 3;
    const int64_t* o = i < 3 ? offs + EO * i : offs + o_mfn + 4 * m;
    seq_fill(E.seq, params + o[0], params + o[1], params + o[2], params + o[3], i < 3 ? S.z[i] : S.hm[m], 0);
    E.seq.gates = w0; w0 += F.W.gates[i];
    if (i < 3)
      for (int l = 0; l < (S.heads ? 3 : 1); ++l) { E.w[l] = params + o[4 + 2 * l]; E.b[l] = params + o[5 + 2 * l]; }
    F.dd[i] = S.d[m]; F.col[i] = m == 0 ? 0 : (m == 1 ? S.d[0] : S.d[0] + S.d[1]);
  }
  w0 = rest;
  for (int m = 0; m < 3; ++m) { P.d[3 + m].seq.cs = w0; A.cs[m] = w0; w0 += F.W.cs[m]; }
  for (int m = 0; m < 3; ++m) { P.d[3 + m].h_last = w0; Mm.hl[m] = w0; w0 += F.W.hl[m]; }
  A.chat = w0; w0 += F.W.chat;
  A.g1p = w0; w0 += F.W.g1p;
  A.g2p = w0; w0 += F.W.g2p;
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
  // gates_e[t][i][g][u] = x_e[t][n0 + i] . W_ih[g h + u] + b_ih + b_hh; pad units u >= h exact zeros
  const bool whole = n == N;           // one chunk: the T * N rows of x are one matrix
  int rc = gemm_group_each(EMFN_LSTMS * (whole ? 1 : T), stream, [&](int p, MfmGemmDesc& d) {
    const int e = p % EMFN_LSTMS, t = p / EMFN_LSTMS;
    const SeqDev& s = P.d[e].seq;
    xproj_desc(d, s, x + ((int64_t)t * N + n0) * D + F.col[e], D, F.dd[e], whole ? T * n : n, s.gates + (int64_t)t * n * 4 * s.Hp);
  });
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
