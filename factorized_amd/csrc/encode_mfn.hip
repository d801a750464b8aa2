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
// Launches 3 and 4 live in encode_mfn_dev.h: mfm_predict_zeros_mfn (zeros_mfn.hip) runs them too, on another gather.
#include "encode_mfn_dev.h"

namespace mfm {

struct EmfnOne {
  SeqDev seq;                                  // gates (the x-projections, read only), w_hh, h, Hp, hk4; an MFN LSTM: cs [T, n, Hp]
  const float* w[3]; const float* b[3];        // an encoder: fc1, the mean head, the logvar head
  float* mu; float* lv;                        // an encoder: this chunk's rows [n, h] (no heads: mu takes fc1's output)
  float* h_last;                               // an MFN LSTM: this chunk's last hidden states [n, h]
  int block_begin;
};
struct EmfnSeqDev { EmfnOne d[EMFN_LSTMS]; int count, T, n, maxw, heads; };

// MFN0: the LSTM at index 0 is one of the MFN's (the launches of one LSTM each); indices 3 .. 5 always are
template <int R, bool MFN0, int K0, int K1, int K2, int K3, int K4, int K5>
__global__ __launch_bounds__(1024) void encode_mfn_seq_kernel(const EmfnSeqDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, bid = blockIdx.x;
  MFM_SEQ_BLOCK_LSTM(P, bid, di)
  const EmfnOne& E = P.d[di];
  const int tile = bid - E.block_begin, b0 = tile * R;
  const int h = E.seq.h;
  const float* hT = nullptr;
  if ((MFN0 && di == 0) || di >= 3) {
    if constexpr (MFN0) { MFM_TUPLE_ONE(0, K0, (hT = small_fwd_body<KQ, R, false, false, false, false, true>(E.seq, P.T, P.n, tile, lds))) }
    MFM_TUPLE_ONE(3, K3, (hT = small_fwd_body<KQ, R, false, false, false, false, true>(E.seq, P.T, P.n, tile, lds)))
    MFM_TUPLE_ONE(4, K4, (hT = small_fwd_body<KQ, R, false, false, false, false, true>(E.seq, P.T, P.n, tile, lds)))
    MFM_TUPLE_ONE(5, K5, (hT = small_fwd_body<KQ, R, false, false, false, false, true>(E.seq, P.T, P.n, tile, lds)))
    store_rows<R>(hT, E.h_last, h, b0, P.n, tid);
    return;
  }
  if constexpr (!MFN0) { MFM_TUPLE_ONE(0, K0, (hT = small_fwd_body<KQ, R, false, false, false>(E.seq, P.T, P.n, tile, lds))) }
  MFM_TUPLE_ONE(1, K1, (hT = small_fwd_body<KQ, R, false, false, false>(E.seq, P.T, P.n, tile, lds)))
  MFM_TUPLE_ONE(2, K2, (hT = small_fwd_body<KQ, R, false, false, false>(E.seq, P.T, P.n, tile, lds)))
  // the two h buffers stay where they are; fc1's output and the two heads' behind them ([maxw][R] each)
  float* act0 = lds + 2 * E.seq.Hp * R;
  float* act1 = act0 + P.maxw * R;
  float* act2 = act1 + P.maxw * R;
  dense_rows<R>(E.w[0], E.b[0], h, h, hT, act0, false);
  if (!P.heads) {
    store_rows<R>(act0, E.mu, h, b0, P.n, tid);
    return;
  }
  dense_rows<R>(E.w[1], E.b[1], h, h, act0, act1, false);
  dense_rows<R>(E.w[2], E.b[2], h, h, act0, act2, false);
  store_rows<R>(act1, E.mu, h, b0, P.n, tid);
  store_rows<R>(act2, E.lv, h, b0, P.n, tid);
}

// ---------------------------------------------------------------- host
static const int kEmfnCanon[EMFN_LSTMS] = {8, 2, 20, 22, 16, 12};      // encoders h = 32 / 8 / 80, the MFN's LSTMs h = 88 / 64 / 48

// the parts of the workspace, in floats, for chunks of `rows` rows
struct EmfnWs { int64_t gates[EMFN_LSTMS], cs[3], hl[3], chat, g1p, g2p, total; };
static void emfn_ws(const EmfnSizes& S, int64_t T, int64_t rows, EmfnWs& W) {
  W.total = 0;
  for (int i = 0; i < EMFN_LSTMS; ++i) { W.gates[i] = rows * T * 4 * hp_of(i < 3 ? S.z[i] : S.hm[i - 3]); W.total += W.gates[i]; }
  for (int m = 0; m < 3; ++m) { W.cs[m] = rows * T * hp_of(S.hm[m]); W.hl[m] = up4(rows * S.hm[m]); W.total += W.cs[m] + W.hl[m]; }
  W.chat = up4(rows * T * S.M); W.g1p = up4(rows * T * S.H1); W.g2p = up4(rows * T * S.H2);
  W.total += W.chat + W.g1p + W.g2p;
}

template <int R>
static int emfn_seq_launch(EmfnSeqDev& P, int threads, size_t lds_bytes, hipStream_t stream) {
  static const char* who = "encode mfn";
  static const char* name = "encode_mfn_seq_kernel";
  bool canon = true;
  for (int i = 0; i < EMFN_LSTMS; ++i) canon = canon && P.d[i].seq.hk4 == kEmfnCanon[i];
  const int tiles = cdiv(P.n, R);
  if (canon) {
    for (int i = 0; i < EMFN_LSTMS; ++i) P.d[i].block_begin = i * tiles;
    return seq_launch_kernel(encode_mfn_seq_kernel<R, false, 8, 2, 20, 22, 16, 12>, name, dim3(EMFN_LSTMS * tiles), dim3(threads), lds_bytes,
                             stream, nullptr, P);
  }
  // other sizes: one launch per LSTM of the kernel instantiated for its size alone (the launch rules of infer_dev.h)
  for (int i = 0; i < EMFN_LSTMS; ++i) {
    EmfnSeqDev Q = P;
    Q.d[0] = P.d[i]; Q.d[0].block_begin = 0; Q.count = 1;
    const int th = std::max(8 * Q.d[0].seq.Hp, 64);
    const int rc = (i < 3)
      ? infer_launch_hk4(who, name, Q.d[0].seq, [](auto kk) { return encode_mfn_seq_kernel<R, false, decltype(kk)::value, 0, 0, 0, 0, 0>; }, Q, tiles, th, lds_bytes, stream)
      : infer_launch_hk4(who, name, Q.d[0].seq, [](auto kk) { return encode_mfn_seq_kernel<R, true, decltype(kk)::value, 0, 0, 0, 0, 0>; }, Q, tiles, th, lds_bytes, stream);
    if (rc != MFM_OK) return rc;
  }
  return MFM_OK;
}

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
  if ((rc = infer_check_rows(who, N, max_rows)) != MFM_OK) return rc;
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
  // the attention chain and the memory recurrence (encode_mfn_dev.h)
  EmfnChain C;
  if ((rc = emfn_chain_check(who, S, (int64_t)T * rows, C)) != MFM_OK) return rc;
  EmfnAttDev& A = C.A;
  EmfnMemDev& Mm = C.Mm;
  if ((rc = infer_check_chunk(who, rows, T, std::max(std::max(D, 4 * round_up(maxw, 16)), std::max(S.M, std::max(S.H1, S.H2))), "projection")) != MFM_OK) return rc;

  // ---- everything that does not depend on the chunk
  EmfnWs W;
  emfn_ws(S, T, rows, W);
  EmfnSeqDev P;
  memset(&P, 0, sizeof(P));
  float* w0 = ws;
  int col[EMFN_LSTMS], dd[EMFN_LSTMS];
  for (int i = 0; i < EMFN_LSTMS; ++i) {
    EmfnOne& E = P.d[i];
    const int m = i % 3;
    const int64_t* o = i < 3 ? offs + EO * i : offs + o_mfn + 4 * m;
    seq_fill(E.seq, params + o[0], params + o[1], params + o[2], params + o[3], i < 3 ? S.z[i] : S.hm[m], 0);
    E.seq.gates = w0; w0 += W.gates[i];
    if (i < 3)
      for (int l = 0; l < (S.heads ? 3 : 1); ++l) { E.w[l] = params + o[4 + 2 * l]; E.b[l] = params + o[5 + 2 * l]; }
    dd[i] = S.d[m]; col[i] = m == 0 ? 0 : (m == 1 ? S.d[0] : S.d[0] + S.d[1]);
  }
  for (int m = 0; m < 3; ++m) { P.d[3 + m].seq.cs = w0; A.cs[m] = w0; w0 += W.cs[m]; }
  for (int m = 0; m < 3; ++m) { P.d[3 + m].h_last = w0; Mm.hl[m] = w0; w0 += W.hl[m]; }
  A.chat = w0; w0 += W.chat;
  A.g1p = w0; w0 += W.g1p;
  A.g2p = w0; w0 += W.g2p;
  P.count = EMFN_LSTMS; P.T = T; P.maxw = maxw; P.heads = S.heads;
  emfn_chain_fill(C, S, T, params, offs + o_att, offs + o_zy, S.heads ? 2 : 1);

  for (int64_t n0 = 0; n0 < N; n0 += rows) {
    const int n = (int)std::min<int64_t>(rows, N - n0);
    // gates_e[t][i][g][u] = x_e[t][n0 + i] . W_ih[g h + u] + b_ih + b_hh; pad units u >= h exact zeros
    const bool whole = n == N;           // one chunk: the T * N rows of x are one matrix
    rc = gemm_group_each(EMFN_LSTMS * (whole ? 1 : T), stream, [&](int p, MfmGemmDesc& d) {
      const int e = p % EMFN_LSTMS, t = p / EMFN_LSTMS;
      const SeqDev& s = P.d[e].seq;
      xproj_desc(d, s, x + ((int64_t)t * N + n0) * D + col[e], D, dd[e], whole ? T * n : n, s.gates + (int64_t)t * n * 4 * s.Hp);
    });
    if (rc != MFM_OK) return rc;
    P.n = n;
    for (int i = 0; i < 3; ++i) { P.d[i].mu = out[i] + n0 * S.z[i]; P.d[i].lv = S.heads ? out[4 + i] + n0 * S.z[i] : nullptr; }
    rc = (R == 1) ? emfn_seq_launch<1>(P, threads, seq_lds, stream) : emfn_seq_launch<4>(P, threads, seq_lds, stream);
    if (rc != MFM_OK) return rc;
    Mm.oz[0] = out[3] + n0 * S.zy;
    Mm.oz[1] = S.heads ? out[7] + n0 * S.zy : nullptr;
    if ((rc = emfn_chain_launch<false>(C, T, n, stream)) != MFM_OK) return rc;
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
