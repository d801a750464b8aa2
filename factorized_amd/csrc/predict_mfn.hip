// Prediction-only path of MFM_KL and MFM (include/mfm_hip.h, mfm_predict_mfn): what mfm_predict_klef (predict.hip) is for
// MFM_KL_EF, for the classes whose label factor comes from the Memory Fusion Network (mfm_model.py:140-199, :723-743) -- y_hat
// and, with labels, the mean L1 / cross-entropy loss, on what they depend on alone:
//   x -> MFN lstm_l / a / v -> attention chain -> memory recurrence -> zy = last_to_zy_fc1([h_l | h_a | h_v | mem]) (the mean)
//     -> fy = relu(zy_to_fy_fc2(relu(zy_to_fy_fc1(zy)))) -> y_hat = fy_to_y_fc2(relu(fy_to_y_fc1(fy)))
// The three modality encoders and their heads, every log-variance head, KLD / MMD, the modalities' z -> f MLPs, the decoders and
// their fc1 reach neither result and do not run; nothing a backward would read is stored.  Per row chunk of n rows, on one stream:
//   1. the input projections of the MFN's lstm_l / a / v on their column ranges of x as ONE grouped fp32 GEMM (a chunk that is
//      not the whole split: one problem per LSTM and time step);
//   2. predict_mfn_seq_kernel, ONE launch: workgroup (MFN LSTM m, row tile) runs the T-step recurrence and stores the cell states
//      c_t and the last h (small_fwd_body's CS mode) -- the MFN branch of encode_mfn_seq_kernel and nothing else;
//   3. encode_mfn_att_kernel<.., ZC = false> (encode_mfn_dev.h) row-wise over the T n pairs (t, row i);
//   4. encode_mfn_mem_kernel<.., ZC = false, TAIL = true>: the memory recurrence per row, last_to_zy_fc1 with zy kept in LDS, the
//      four small layers behind it in the same workgroup -> the row of y_hat and, with labels, the row's loss contribution.
// Loss: the arrival ticket of predict_klef_kernel, per chunk -- the workgroup that draws the chunk's last ticket adds the chunk's
// contributions in a fixed order in fp64 onto the running sum of the chunks before it, and behind the last chunk divides by the
// counts of the WHOLE split; one ticket word, put back to 0 by every last arriver.  No float atomics touch the result, nobody
// waits or spins: y_hat and the loss are bit-identical from run to run for a given (T, N, max_rows); a row's arithmetic does not
// depend on its place in a tile or a chunk, so y_hat is bit-identical for every chunking within one tile-row form of launch 2.
// Launch 2 follows the launch rules of infer_dev.h: the per-block switch for the canonical size tuple only, else one launch per LSTM.
// The host side of launches 1, 3 and 4, the size parser, the refusals and the workspace parts behind the projections are the
// shared ones of encode_mfn_dev.h (its file head lists them); here: launch 2, the tail's arguments and the loss words.
#include "encode_mfn_dev.h"

namespace mfm {

#define PMFN_LSTMS 3
#define PMFN_OFFS 38          // 12 of the MFN's LSTM cells, 16 of its attention and gamma networks, 2 of last_to_zy_fc1, 8 of the tail

struct PmfnOne {
  SeqDev seq;                                  // gates (the x-projections, read only), w_hh, h, Hp, hk4; cs [T, n, Hp]
  float* h_last;                               // this chunk's last hidden states [n, h]
  int block_begin;
};
struct PmfnSeqDev { PmfnOne d[PMFN_LSTMS]; int count, T, n; };

template <int R, int K0, int K1, int K2>
__global__ __launch_bounds__(1024) void predict_mfn_seq_kernel(const PmfnSeqDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, bid = blockIdx.x;
  MFM_SEQ_BLOCK_LSTM(P, bid, di)
  const PmfnOne& E = P.d[di];
  const int tile = bid - E.block_begin, b0 = tile * R;
  const float* hT = nullptr;
  MFM_TUPLE3((hT = small_fwd_body<KQ, R, false, false, false, false, true>(E.seq, P.T, P.n, tile, lds)))
  store_rows<R>(hT, E.h_last, E.seq.h, b0, P.n, tid);
}

// ---------------------------------------------------------------- host
static const int kPmfnCanon[PMFN_LSTMS] = {22, 16, 12};      // the MFN's LSTMs h = 88 / 64 / 48

// the workspace, in this order (every part a multiple of 4 floats; include/mfm_hip.h states it term by term): the chunk's three
// x-projections; the parts of mfn_ws; one loss contribution per chunk row; the fp64 running sum, the ticket word and a pad
struct PmfnLayout { int64_t o_cs, o_row, o_acc, total; };
static PmfnLayout pmfn_layout(const EmfnSizes& S, int64_t T, int64_t N, int64_t max_rows) {
  const int64_t rows = gen_rows(N, max_rows);
  PmfnLayout L;
  L.o_cs = 0;
  for (int m = 0; m < PMFN_LSTMS; ++m) L.o_cs += rows * T * 4 * hp_of(S.hm[m]);
  L.o_row = L.o_cs + mfn_ws(S, T, rows, 1).total;
  L.o_acc = L.o_row + up4(rows);
  L.total = L.o_acc + 4;
  return L;
}

template <int R>
static int pmfn_seq_launch(const char* who, PmfnSeqDev& P, int threads, size_t lds_bytes, hipStream_t stream) {
  bool canon = true;
  for (int i = 0; i < PMFN_LSTMS; ++i) canon = canon && P.d[i].seq.hk4 == kPmfnCanon[i];
  return infer_launch_tuple_or_each<R>(who, "predict_mfn_seq_kernel", P, canon ? predict_mfn_seq_kernel<R, 22, 16, 12> : nullptr,
                                       [](auto kk) { return predict_mfn_seq_kernel<R, decltype(kk)::value, 0, 0>; }, threads, lds_bytes, stream);
}

static int predict_mfn(int T, int64_t N, const int32_t* sz, const float* params, const int64_t* offs, const float* x, const void* y,
                       float* ws, float* y_hat, float* loss, int64_t max_rows, hipStream_t stream) {
  static const char* who = "predict mfn";
  MfnSizes Z;      // (the encoders' z sizes, fl / fa / fv and heads: checked, otherwise unused)
  MFM_REQUIRE(T >= 1 && N >= 1 && mfn_sizes(sz, Z),
              "%s: sizes must be positive (T %d, N %lld, and the %d sizes; heads and the loss kind 0 or 1)", who, T, (long long)N, MFN_SIZES);
  MFM_REQUIRE(params && offs && x && ws && y_hat, "%s: bad arguments (params, offsets, x, workspace and y_hat must not be null)", who);
  MFM_REQUIRE((y != nullptr) == (loss != nullptr), "%s: labels and loss come together (both, or both null)", who);
  const EmfnSizes& S = Z.E;
  int rc = infer_check_aligned(who, params, x, ws);
  if (rc != MFM_OK) return rc;
  if ((rc = infer_check_rows(who, N, max_rows)) != MFM_OK) return rc;
  const int o_att = 4 * PMFN_LSTMS, o_zy = o_att + 16, o_tail = o_zy + 2;
  if ((rc = infer_check_offsets(who, offs, PMFN_OFFS, 4, 0, o_att)) != MFM_OK) return rc;
  if ((rc = mfn_check_covered(who, S, false)) != MFM_OK) return rc;
  const int hmax = std::max(S.hm[0], std::max(S.hm[1], S.hm[2]));
  const int D = S.d[0] + S.d[1] + S.d[2], od = Z.od, loss_kind = Z.loss_kind;
  const int tailw = round_up(std::max(S.zy, std::max(Z.fy, od)), 4);      // the widest activation of the tail
  const int rows = (int)gen_rows(N, max_rows);
  const int R = gen_tile_rows(PMFN_LSTMS, rows);
  const int threads = std::max(64, 8 * round_up(hmax, 16));
  size_t seq_floats = 0;
  for (int m = 0; m < PMFN_LSTMS; ++m) seq_floats = std::max(seq_floats, seq_lds_floats(S.hm[m], R));
  const size_t seq_lds = lds_bytes_of(seq_floats);
  if ((rc = infer_check_lds(who, seq_lds, hmax, R)) != MFM_OK) return rc;
  EmfnChain C;
  if ((rc = emfn_chain_check(who, S, (int64_t)T * rows, C, tailw)) != MFM_OK) return rc;
  if ((rc = infer_check_chunk(who, rows, T, std::max(std::max(D, 4 * round_up(hmax, 16)), std::max(S.M, std::max(S.H1, S.H2))), "projection")) != MFM_OK)
    return rc;

  // ---- everything that does not depend on the chunk
  const PmfnLayout lay = pmfn_layout(S, T, N, max_rows);
  PmfnSeqDev P;
  memset(&P, 0, sizeof(P));
  emfn_chain_fill(C, S, T, params, offs + o_att, offs + o_zy, 1);
  MfnLstm L[PMFN_LSTMS];
  for (int m = 0; m < PMFN_LSTMS; ++m) L[m] = MfnLstm{&P.d[m].seq, &P.d[m].h_last, 0, 0};
  mfn_lstms_fill(L, C, S, T, rows, 1, params, offs, ws, ws + lay.o_cs);
  P.count = PMFN_LSTMS; P.T = T;

  EmfnTailDev Q;
  memset(&Q, 0, sizeof(Q));
  for (int l = 0; l < 4; ++l) { Q.wt[l] = params + offs[o_tail + 2 * l]; Q.bt[l] = params + offs[o_tail + 2 * l + 1]; }
  Q.rowloss = ws + lay.o_row;
  Q.acc = reinterpret_cast<double*>(ws + lay.o_acc);      // (a multiple of 4 floats from a 16-byte aligned base)
  Q.ticket = reinterpret_cast<int*>(ws + lay.o_acc + 2);
  Q.loss = loss;
  Q.inv = inv_label_count(loss_kind, N, od);
  Q.fy = Z.fy; Q.od = od; Q.loss_kind = loss_kind; Q.tailw = tailw;
  // (a call that ended in an error between two launches may have left arrivals behind)
  if (loss) MFM_HIP_CHECK(hipMemsetAsync(Q.ticket, 0, sizeof(int), stream));

  for (int64_t n0 = 0; n0 < N; n0 += rows) {
    const int n = (int)std::min<int64_t>(rows, N - n0);
    rc = mfn_xproj_chunk(PMFN_LSTMS, L, x, T, N, D, n0, n, stream);
    if (rc != MFM_OK) return rc;
    P.n = n;
    rc = (R == 1) ? pmfn_seq_launch<1>(who, P, threads, seq_lds, stream) : pmfn_seq_launch<4>(who, P, threads, seq_lds, stream);
    if (rc != MFM_OK) return rc;
    if ((rc = emfn_att_launch<false>(C, T, n, stream)) != MFM_OK) return rc;
    static_cast<EmfnMemDev&>(Q) = C.Mm;
    Q.y = labels_at(y, loss_kind, n0, od);
    Q.y_hat = y_hat + n0 * od;
    Q.first = n0 == 0; Q.last = n0 + n == N;
    rc = emfn_mem_launch<false, true>(C, Q, stream);
    if (rc != MFM_OK) return rc;
  }
  return MFM_OK;
}

}  // namespace mfm

extern "C" int64_t mfm_predict_mfn_workspace_floats(int32_t T, int64_t N, const int32_t* sizes, int64_t max_rows) {
  mfm::MfnSizes Z;
  if (T < 1 || N < 1 || max_rows < 0 || !sizes || !mfm::mfn_sizes(sizes, Z)) return 0;
  return mfm::pmfn_layout(Z.E, T, N, max_rows).total;
}

extern "C" int mfm_predict_mfn_tile_rows(int64_t N, int64_t max_rows) {
  if (N < 1 || max_rows < 0) return -1;
  return mfm::gen_tile_rows(PMFN_LSTMS, (int)mfm::gen_rows(N, max_rows));
}

extern "C" int mfm_predict_mfn(int32_t T, int64_t N, const int32_t* sizes, const float* params, const int64_t* offsets, const float* x,
                               const void* y, float* workspace, float* y_hat, float* loss, int64_t max_rows, void* stream) {
  return mfm::predict_mfn(T, N, sizes, params, offsets, x, y, workspace, y_hat, loss, max_rows, (hipStream_t)stream);
}
