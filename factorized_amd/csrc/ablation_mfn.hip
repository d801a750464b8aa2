// Prediction of the ablations M_A and M_C (include/mfm_hip.h, mfm_predict_ablation_mfn): what the `evaluate` / `predict` blocks of
// the reference's train_mfm_ablation report for the two classes whose label factor comes from the Memory Fusion Network -- y_hat,
// its label loss and the three reconstruction errors -- on what those numbers depend on alone (no MMD, no x_hat written):
//   family 0, M_A   zy = last_to_zy_fc1(MFN(x)); fy = relu(zy_to_fy_fc2(relu(zy_to_fy_fc1(zy)))); y_hat = fy_to_y_fc2(relu(fy_to_y_fc1(fy)));
//                   zl = encoder_l(x) over ALL D columns; fl = relu(zl_to_fl_fc2(relu(zl_to_fl_fc1(zl))));
//                   gen_m = mse(decoder_m([fy | fl], T), x_m)
//   family 1, M_C   the same label path; gen_m = mse(decoder_m(fy, T), x_m)
// Everything but the wiring is shared.  Per row chunk, on one stream:
//   1. the input projections of the MFN's lstm_l / a / v on their column ranges of x and, family 0 with gen, of encoder_l on all
//      of x, as ONE grouped GEMM (mfn_xproj_chunk, infer_dev.h);
//   2. ablation_mfn_seq_kernel, ONE launch of (LSTM, row tile) workgroups: an MFN block is predict_mfn_seq_kernel's body (cell
//      states and last h stored); the block of encoder_l is ablation_encode_kernel's (recurrence, fc1 and the zl -> fl MLP on
//      chip), which stores its fl rows into columns [fy, fy + fl) of the chunk's embedding block [n, fy + fl]; zl never leaves
//      the chip;
//   3. the attention chain of mfm_encode_mfn (emfn_att_launch<false>, encode_mfn_dev.h);
//   4. encode_mfn_mem_kernel<.., TAIL> as mfm_predict_mfn launches it -- y_hat, the row's loss contribution, the chunk's
//      ticket --, with gen its EMB form, which also stores the row's fy into columns [0, fy) of the embedding block;
//   5. with gen: ablation_decode_kernel (ablation_dec_dev.h), ONE launch of (decoder m, row tile) workgroups that all stage the
//      same embedding rows and store h_t; fc1_sqerr_kernel (objective.hip) over the stored h against x, one partial per
//      workgroup; zeros_finish_kernel (zeros.hip) adds the partials in fp64 in a fixed order.
// Nobody waits or spins; the only ticket is the loss ticket of launch 4; no float atomics touch a result.  The MFN blocks' tile
// rows come from the MFN's three LSTMs alone whatever with_gen, and launch 4 is the same arithmetic with and without EMB: y_hat
// and disc have the same bits with and without gen.  Launch 2 follows the launch rules of infer_dev.h: the per-block switch for
// the canonical size tuple only (MFN h = 88 / 64 / 48, encoder_l h = 32), else one launch per LSTM.  The three decoders have one
// hidden size, so launch 5 is one launch of the kernel instantiated for that size alone, whatever the size.
#include "encode_mfn_dev.h"
#include "ablation_dec_dev.h"

namespace mfm {

#define AMFN_FAMILIES 2
#define AMFN_LSTMS 4          // the MFN's lstm l, a, v, then encoder_l (family 0 with gen)
// the parameter table: the 38 of mfm_predict_mfn in its offset order, 18 of decoder_l / a / v, 10 of encoder_l and zl_to_fl
#define AMFN_P_ATT 12
#define AMFN_P_ZY 28
#define AMFN_P_TAIL 30
#define AMFN_P_DEC 38
#define AMFN_P_ENC 56
#define AMFN_NPARAM 66

struct AmfnOne {
  SeqDev seq;                                  // gates (the x-projections, read only), w_hh, h, Hp, hk4; an MFN LSTM: cs [T, n, Hp]
  float* h_last;                               // an MFN LSTM: this chunk's last hidden states [n, h]
  const float* w[3]; const float* b[3];        // encoder_l: its fc1, zl_to_fl fc1, fc2
  int block_begin;
};
struct AmfnSeqDev {
  AmfnOne d[AMFN_LSTMS];
  float* emb;                                  // workspace: this chunk's embedding block [n, embw]; fl at columns [col, col + fl)
  int count, T, n, maxw, fl, embw, col;
};

// ENC0: the LSTM at index 0 is encoder_l (the launches of one LSTM each); index 3 always is
template <int R, bool ENC0, int K0, int K1, int K2, int K3>
__global__ __launch_bounds__(1024) void ablation_mfn_seq_kernel(const AmfnSeqDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, bid = blockIdx.x;
  MFM_SEQ_BLOCK_LSTM(P, bid, di)
  const AmfnOne& E = P.d[di];
  const int tile = bid - E.block_begin, b0 = tile * R;
  const float* hT = nullptr;
  if ((ENC0 && di == 0) || di == 3) {
    if constexpr (ENC0) { MFM_TUPLE_ONE(0, K0, (hT = small_fwd_body<KQ, R, false, false, false>(E.seq, P.T, P.n, tile, lds))) }
    MFM_TUPLE_ONE(3, K3, (hT = small_fwd_body<KQ, R, false, false, false>(E.seq, P.T, P.n, tile, lds)))
    // the two h buffers stay where they are; two activations behind them ([maxw][R] each): zl and fl in the first, the MLP's
    // hidden layer in the second
    float* act0 = lds + 2 * E.seq.Hp * R;
    float* act1 = act0 + P.maxw * R;
    const int h = E.seq.h, fl = P.fl;
    dense_rows<R>(E.w[0], E.b[0], h, h, hT, act0, false);
    dense_rows<R>(E.w[1], E.b[1], h, fl, act0, act1, true);
    dense_rows<R>(E.w[2], E.b[2], fl, fl, act1, act0, true);
    for (int e = tid; e < fl * R; e += blockDim.x) {
      const int r = e / fl, o = e - r * fl;
      if (b0 + r < P.n) P.emb[(int64_t)(b0 + r) * P.embw + P.col + o] = act0[o * R + r];
    }
    return;
  }
  if constexpr (!ENC0) { MFM_TUPLE_ONE(0, K0, (hT = small_fwd_body<KQ, R, false, false, false, false, true>(E.seq, P.T, P.n, tile, lds))) }
  MFM_TUPLE_ONE(1, K1, (hT = small_fwd_body<KQ, R, false, false, false, false, true>(E.seq, P.T, P.n, tile, lds)))
  MFM_TUPLE_ONE(2, K2, (hT = small_fwd_body<KQ, R, false, false, false, false, true>(E.seq, P.T, P.n, tile, lds)))
  store_rows<R>(hT, E.h_last, E.seq.h, b0, P.n, tid);
}

// ---------------------------------------------------------------- host
static const int kAmfnCanon[AMFN_LSTMS] = {22, 16, 12, 8};      // the MFN's LSTMs h = 88 / 64 / 48, encoder_l h = 32

// the launch(es) of the recurrences on a chunk of P.n rows: P.d[0 .. P.count) filled but for block_begin, P.count 3 or 4
template <int R>
static int amfn_seq_launch(const char* who, AmfnSeqDev& P, int threads, size_t lds_bytes, hipStream_t stream) {
  static const char* name = "ablation_mfn_seq_kernel";
  bool canon = true;
  for (int i = 0; i < P.count; ++i) canon = canon && P.d[i].seq.hk4 == kAmfnCanon[i];
  const int tiles = cdiv(P.n, R);
  if (canon) {
    for (int i = 0; i < P.count; ++i) P.d[i].block_begin = i * tiles;
    return seq_launch_kernel(ablation_mfn_seq_kernel<R, false, 22, 16, 12, 8>, name, dim3(P.count * tiles), dim3(threads), lds_bytes, stream,
                             nullptr, P);
  }
  // other sizes: one launch per LSTM of the kernel instantiated for its size alone (the launch rules of infer_dev.h)
  for (int i = 0; i < P.count; ++i) {
    AmfnSeqDev Q = P;
    Q.d[0] = P.d[i]; Q.d[0].block_begin = 0; Q.count = 1;
    const int th = std::max(8 * Q.d[0].seq.Hp, 64);
    const int rc = (i < 3)
      ? infer_launch_hk4(who, name, Q.d[0].seq, [](auto kk) { return ablation_mfn_seq_kernel<R, false, decltype(kk)::value, 0, 0, 0>; }, Q, tiles, th, lds_bytes, stream)
      : infer_launch_hk4(who, name, Q.d[0].seq, [](auto kk) { return ablation_mfn_seq_kernel<R, true, decltype(kk)::value, 0, 0, 0>; }, Q, tiles, th, lds_bytes, stream);
    if (rc != MFM_OK) return rc;
  }
  return MFM_OK;
}

// the sizes of a call from the 23 of mfm_predict_zeros_mfn: zl and fl count for family 0 alone; w: the decoders' hidden size
struct AmfnSizes { MfnSizes Z; int zl, fl, w; };
static bool amfn_sizes(const int32_t* sz, int family, AmfnSizes& A) {
  if (!sz || !mfn_sizes(sz, A.Z)) return false;
  A.zl = sz[3]; A.fl = sz[17];
  A.w = family == 0 ? A.Z.fy + A.fl : A.Z.fy;
  return true;
}

// the workspace, in this order (every part a multiple of 4 floats; include/mfm_hip.h states it term by term): the chunk's
// x-projections (the MFN's three, then encoder_l's); the parts of mfn_ws; the embedding block; with gen the decoders' stored h, the
// squared-error partials and the ZER_ACC fp64 accumulators; with labels one loss contribution per chunk row; the fp64 running
// sum, the ticket word and a pad
struct AmfnLayout { int64_t o_enc, o_cs, o_emb, o_hs, o_part, o_acc, o_row, o_tail, total; };
static AmfnLayout amfn_layout(const AmfnSizes& A, int64_t T, int64_t N, int family, bool with_gen, bool with_labels, int64_t max_rows) {
  const EmfnSizes& S = A.Z.E;
  const int64_t rows = gen_rows(N, max_rows);
  AmfnLayout L;
  L.o_enc = 0;
  for (int m = 0; m < 3; ++m) L.o_enc += rows * T * 4 * hp_of(S.hm[m]);
  L.o_cs = L.o_enc + ((family == 0 && with_gen) ? rows * T * 4 * hp_of(A.zl) : 0);
  L.o_emb = L.o_cs + mfn_ws(S, T, rows, 1).total;
  L.o_hs = L.o_emb + up4(rows * A.w);
  L.o_part = L.o_hs + (with_gen ? ABL_MODS * rows * T * hp_of(A.w) : 0);
  L.o_acc = L.o_part + (with_gen ? up4(fc1_sqerr_tiles(T, rows, S.d)) : 0);
  L.o_row = L.o_acc + (with_gen ? up4(2 * ZER_ACC) : 0);
  L.o_tail = L.o_row + (with_labels ? up4(rows) : 0);
  L.total = L.o_tail + 4;
  return L;
}

// rows per workgroup of the recurrence launch and of the decoders' (0: none): the MFN's three LSTMs alone decide the first,
// whatever with_gen -- y_hat and disc must not depend on it
static void amfn_tile_rows(bool with_gen, int rows, int* Rs, int* Rd) {
  *Rs = gen_tile_rows(3, rows);
  *Rd = with_gen ? gen_tile_rows(ABL_MODS, rows) : 0;
}

static int predict_ablation_mfn(int T, int64_t N, const int32_t* sz, int family, int with_gen, const float* const* prm, const float* x,
                                const void* y, float* ws, float* y_hat, float* gen, float* disc, int64_t max_rows, hipStream_t stream) {
  static const char* who = "predict ablation mfn";
  MFM_REQUIRE(sz && prm && x && ws && y_hat, "%s: bad arguments (sizes, parameter table, x, workspace and y_hat must not be null)", who);
  MFM_REQUIRE(family >= 0 && family < AMFN_FAMILIES, "%s: family = %d (0 M_A, 1 M_C)", who, family);
  AmfnSizes A;
  MFM_REQUIRE(T >= 1 && N >= 1 && amfn_sizes(sz, family, A),
              "%s: sizes must be positive (T %d, N %lld, and the %d sizes; heads and the loss kind 0 or 1)", who, T, (long long)N, MFN_SIZES);
  int rc = infer_check_rows(who, N, max_rows);
  if (rc != MFM_OK) return rc;
  MFM_REQUIRE(with_gen == 0 || with_gen == 1, "%s: with_gen = %d (0 or 1)", who, with_gen);
  MFM_REQUIRE((with_gen != 0) == (gen != nullptr), "%s: with_gen and gen come together (both, or neither)", who);
  MFM_REQUIRE((y != nullptr) == (disc != nullptr), "%s: labels and disc come together (both, or both null)", who);
  const EmfnSizes& S = A.Z.E;
  const int od = A.Z.od, fy = A.Z.fy, loss_kind = A.Z.loss_kind, w = A.w;
  const bool enc = family == 0 && with_gen;
  // (x is read 16 bytes at a time by the grouped GEMM alone, which takes dword-aligned addresses, and element by element as the
  // squared error's target; the recurrences read the workspace 16 bytes at a time)
  MFM_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)ws & 15) == 0, "%s: x must be 4-byte aligned, the workspace 16-byte aligned", who);
  MFM_REQUIRE((((uintptr_t)y_hat | (uintptr_t)gen | (uintptr_t)disc) & 3) == 0 && ((uintptr_t)y & (loss_kind == 0 ? 3 : 7)) == 0,
              "%s: y_hat, gen, disc or the labels are misaligned", who);
  for (int i = 0; i < AMFN_NPARAM; ++i) {
    if (i >= AMFN_P_DEC && !with_gen) break;
    if (i >= AMFN_P_ENC && !enc) break;
    const int j = i < AMFN_P_ATT ? i % 4 : (i >= AMFN_P_DEC && i < AMFN_P_ENC + 6 ? (i - AMFN_P_DEC) % 6 : 2);
    const bool lstm_w = j < 2;
    MFM_REQUIRE(prm[i], "%s: parameter %d is null", who, i);
    MFM_REQUIRE(((uintptr_t)prm[i] & (lstm_w ? 15 : 3)) == 0, "%s: parameter %d is misaligned (LSTM weights 16 bytes, the rest 4)", who, i);
  }

  // ---- the refusals: what mfm_predict_mfn refuses, then the encoder's and the decoders' hidden sizes and the LDS
  if ((rc = mfn_check_covered(who, S, false)) != MFM_OK) return rc;
  if (enc && (rc = infer_check_resident(who, A.zl)) != MFM_OK) return rc;
  if (with_gen && (rc = infer_check_resident(who, w)) != MFM_OK) return rc;
  const int hmax = std::max(S.hm[0], std::max(S.hm[1], S.hm[2]));
  const int hall = enc ? std::max(hmax, A.zl) : hmax;
  const int D = S.d[0] + S.d[1] + S.d[2];
  const int tailw = round_up(std::max(S.zy, std::max(fy, od)), 4);      // the widest activation of the tail
  const int rows = (int)gen_rows(N, max_rows);
  int R, Rd;
  amfn_tile_rows(with_gen != 0, rows, &R, &Rd);
  const int threads = std::max(64, 8 * round_up(hall, 16));
  const int enc_maxw = std::max(A.zl, A.fl);
  size_t seq_floats = 0;
  for (int m = 0; m < 3; ++m) seq_floats = std::max(seq_floats, seq_lds_floats(S.hm[m], R));
  if (enc) seq_floats = std::max(seq_floats, enc_lds_floats(A.zl, R, 2, enc_maxw));
  const size_t seq_lds = lds_bytes_of(seq_floats);
  if ((rc = infer_check_lds(who, seq_lds, enc ? std::max(hmax, enc_maxw) : hmax, R)) != MFM_OK) return rc;
  const size_t dec_seq = with_gen ? seq_lds_floats(w, Rd) : 0;
  const size_t dec_lds = with_gen ? lds_bytes_of(dec_seq + (size_t)w * Rd) : 0;
  if (with_gen && (rc = infer_check_lds(who, dec_lds, w, Rd)) != MFM_OK) return rc;
  EmfnChain C;
  if ((rc = emfn_chain_check(who, S, (int64_t)T * rows, C, tailw)) != MFM_OK) return rc;
  if ((rc = infer_check_chunk(who, rows, T, std::max(std::max(D, 4 * round_up(hall, 16)), std::max(S.M, std::max(S.H1, S.H2))), "projection")) != MFM_OK)
    return rc;
  MFM_REQUIRE((int64_t)rows * w < ((int64_t)1 << 31), "%s: a chunk of %d rows is too large; pass a row cap", who, rows);
  MFM_REQUIRE(!with_gen || fc1_sqerr_tiles(T, rows, S.d) < ((int64_t)1 << 31), "%s: a chunk of %d rows x %d steps is too large; pass a row cap", who, rows, T);

  // ---- everything that does not depend on the chunk
  const AmfnLayout lay = amfn_layout(A, T, N, family, with_gen != 0, y != nullptr, max_rows);
  AmfnSeqDev P;
  AblDecDev PD;
  Fc1SqLaunch Sq;
  memset(&P, 0, sizeof(P));
  memset(&PD, 0, sizeof(PD));
  memset(&Sq, 0, sizeof(Sq));
  emfn_chain_fill_ptrs(C, S, T, prm + AMFN_P_ATT, prm + AMFN_P_ZY, 1);
  MfnLstm L[AMFN_LSTMS];
  for (int m = 0; m < 3; ++m) L[m] = MfnLstm{&P.d[m].seq, &P.d[m].h_last, 0, 0};
  mfn_lstms_fill_ptrs(L, C, S, T, rows, 1, prm, ws, ws + lay.o_cs);
  float* emb = ws + lay.o_emb;
  P.count = 3; P.T = T;
  if (enc) {
    const float* const* p = prm + AMFN_P_ENC;
    AmfnOne& E = P.d[3];
    seq_fill(E.seq, p[0], p[1], p[2], p[3], A.zl, 0);
    E.seq.gates = ws + lay.o_enc;
    for (int l = 0; l < 3; ++l) { E.w[l] = p[4 + 2 * l]; E.b[l] = p[5 + 2 * l]; }
    L[3] = MfnLstm{&E.seq, nullptr, 0, D};      // (all D columns of x)
    P.count = AMFN_LSTMS; P.emb = emb; P.maxw = enc_maxw; P.fl = A.fl; P.embw = w; P.col = fy;
  }

  EmfnTailDev Q;
  memset(&Q, 0, sizeof(Q));
  for (int l = 0; l < 4; ++l) { Q.wt[l] = prm[AMFN_P_TAIL + 2 * l]; Q.bt[l] = prm[AMFN_P_TAIL + 2 * l + 1]; }
  Q.rowloss = ws + lay.o_row;
  Q.acc = reinterpret_cast<double*>(ws + lay.o_tail);      // (a multiple of 4 floats from a 16-byte aligned base)
  Q.ticket = reinterpret_cast<int*>(ws + lay.o_tail + 2);
  Q.loss = disc;
  Q.inv = inv_label_count(loss_kind, N, od);
  Q.fy = fy; Q.od = od; Q.loss_kind = loss_kind; Q.tailw = tailw;
  Q.emb = with_gen ? emb : nullptr; Q.embw = w;

  ZerFinishDev Fin;
  memset(&Fin, 0, sizeof(Fin));
  if (with_gen) {
    float* hs = ws + lay.o_hs;
    Sq.hmax = w;
    for (int m = 0; m < ABL_MODS; ++m) {
      const float* const* p = prm + AMFN_P_DEC + 6 * m;
      AblDec& Dd = PD.d[m];
      seq_fill(Dd.seq, p[0], p[1], p[2], p[3], w, 1);
      Dd.seq.hs = hs; hs += (int64_t)rows * T * Dd.seq.Hp;
      Dd.col = 0;      // (the three decoders read the same embedding)
      Fc1SqItem& I = Sq.F.it[m];
      I.hs = Dd.seq.hs; I.w = p[4]; I.bias = p[5];
      I.d = S.d[m]; I.h = w; I.Hp = Dd.seq.Hp; I.col_tiles = cdiv(S.d[m], OBJ_BN);
      Sq.col[m] = mfn_col(S, m);
      Sq.inv_gen[m] = 1.0 / ((double)T * (double)N * (double)S.d[m]);
      Fin.inv_gen[m] = Sq.inv_gen[m];
    }
    Sq.F.D = D; Sq.F.N = N; Sq.T = T;
    PD.f = emb; PD.count = ABL_MODS; PD.T = T; PD.ftot = w; PD.seq_floats = (int)dec_seq;
    Fin.acc = reinterpret_cast<double*>(ws + lay.o_acc);
    Fin.gen = gen;
    Fin.od = od; Fin.loss_kind = loss_kind;      // (no labels here: the label loss is the ticket's)
  }
  float* part = ws + lay.o_part;
  // (a call that ended in an error between two launches may have left arrivals behind)
  if (disc) MFM_HIP_CHECK(hipMemsetAsync(Q.ticket, 0, sizeof(int), stream));

  for (int64_t n0 = 0; n0 < N; n0 += rows) {
    const int n = (int)std::min<int64_t>(rows, N - n0);
    if ((rc = mfn_xproj_chunk(P.count, L, x, T, N, D, n0, n, stream)) != MFM_OK) return rc;
    P.n = n;
    rc = (R == 1) ? amfn_seq_launch<1>(who, P, threads, seq_lds, stream) : amfn_seq_launch<4>(who, P, threads, seq_lds, stream);
    if (rc != MFM_OK) return rc;
    if ((rc = emfn_att_launch<false>(C, T, n, stream)) != MFM_OK) return rc;
    static_cast<EmfnMemDev&>(Q) = C.Mm;
    Q.y = labels_at(y, loss_kind, n0, od);
    Q.y_hat = y_hat + n0 * od;
    Q.first = n0 == 0; Q.last = n0 + n == N;
    rc = with_gen ? emfn_mem_launch<false, true, true>(C, Q, stream) : emfn_mem_launch<false, true>(C, Q, stream);
    if (rc != MFM_OK) return rc;
    if (!with_gen) continue;
    PD.n = n;
    rc = (Rd == 1) ? abl_decode_launch_same<1>(who, PD, dec_lds, stream) : abl_decode_launch_same<4>(who, PD, dec_lds, stream);
    if (rc != MFM_OK) return rc;
    if ((rc = fc1_sqerr_chunk(Sq, x, n0, n, part, Fin.part, Fin.npart, stream)) != MFM_OK) return rc;
    Fin.n = n; Fin.first = n0 == 0; Fin.last = n0 + n == N;
    if ((rc = zeros_finish_launch(Fin, stream)) != MFM_OK) return rc;
  }
  return MFM_OK;
}

}  // namespace mfm

extern "C" int64_t mfm_predict_ablation_mfn_workspace_floats(int32_t T, int64_t N, const int32_t* sizes, int32_t family, int32_t with_gen,
                                                             int32_t with_labels, int64_t max_rows) {
  mfm::AmfnSizes A;
  if (T < 1 || N < 1 || family < 0 || family >= AMFN_FAMILIES || max_rows < 0 || with_gen < 0 || with_gen > 1 || !mfm::amfn_sizes(sizes, family, A))
    return 0;
  return mfm::amfn_layout(A, T, N, family, with_gen != 0, with_labels != 0, max_rows).total;
}

extern "C" int mfm_predict_ablation_mfn_tile_rows(int64_t N, int32_t family, int32_t with_gen, int64_t max_rows, int32_t* tile_rows) {
  if (N < 1 || max_rows < 0 || !tile_rows || family < 0 || family >= AMFN_FAMILIES || with_gen < 0 || with_gen > 1) {
    mfm::set_error("predict ablation mfn tile rows: bad arguments (N %lld, family %d, with_gen %d, row cap %lld)", (long long)N, family, with_gen,
                   (long long)max_rows);
    return MFM_ERR_ARG;
  }
  const int rows = (int)std::min<int64_t>(mfm::gen_rows(N, max_rows), INT32_MAX);
  int Rs, Rd;
  mfm::amfn_tile_rows(with_gen != 0, rows, &Rs, &Rd);
  tile_rows[0] = Rs; tile_rows[1] = Rd;
  return MFM_OK;
}

extern "C" int mfm_predict_ablation_mfn(int32_t T, int64_t N, const int32_t* sizes, int32_t family, int32_t with_gen,
                                        const float* const* params, const float* x, const void* y, float* workspace, float* y_hat,
                                        float* gen, float* disc, int64_t max_rows, void* stream) {
  return mfm::predict_ablation_mfn(T, N, sizes, family, with_gen, params, x, y, workspace, y_hat, gen, disc, max_rows, (hipStream_t)stream);
}
