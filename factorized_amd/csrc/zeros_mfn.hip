// The zeroed-modality test protocol of MFM_KL and MFM (include/mfm_hip.h, mfm_predict_zeros_mfn): what mfm_predict_zeros_klef
// (zeros.hip) is for MFM_KL_EF, for the classes whose label factor comes from the Memory Fusion Network (mfm_model.py:140-199,
// :723-743) -- the test split through the eval forward three times, each time with one modality's columns set to zero (cases:
// no l, no a, no v); y_hat of every case, F.mse_loss of the ZEROED modality's reconstruction against the real x_c, and the label
// loss per case -- on what those results depend on alone:
//   y_hat_c   <- zy_c = last_to_zy_fc1([h_l | h_a | h_v | mem]) of the MFN on x with modality c's columns zero -> fy -> classifier
//   x_c_hat_c <- decoder_c([fy_c | f_c]) with f_c from z_c^0, encoder_c's factor on zeros: the same row for every sample
// The MFN's three LSTMs are independent of each other: on the real columns they run ONCE for the three cases, and the LSTM of a
// zeroed modality sees the same all-zero row for every sample -- one row of work.  The encoders of the present modalities reach
// none of the results and do not run.  No x is copied or zeroed, no x_hat is written, no log-variance head, no KLD, no MMD.
// Per row chunk of n rows, on one stream:
//   1. the input projections of the MFN's lstm_l / a / v on their column ranges of x as ONE grouped fp32 GEMM (a chunk that is
//      not the whole split: one problem per LSTM and time step);
//   2. zeros_mfn_seq_kernel, ONE launch: workgroup (MFN LSTM m, row tile) runs the T-step recurrence and stores the cell states
//      c_t and the last h (small_fwd_body's CS mode, as encode_mfn_seq_kernel).  In the first chunk six more one-row workgroups
//      run on the constant gates b_ih + b_hh (zeros_mfn_cgates_kernel fills them in front): the three MFN LSTMs on zero input
//      (their one-row c record and last h) and encoder l / a / v on zero input, which go on with fc1 and, with heads ("kl"),
//      the mean head, and write z_c^0 once per row of a chunk (decode_factors_kernel stages its z rows without a stride);
//   3. encode_mfn_att_kernel<.., ZC = true> (encode_mfn_dev.h) row-wise over the 3 T n triples (t, case c, row i): cStar with
//      modality c's columns from the one-row zero record, the others from the real records; the chain on the fp32 MFMA;
//   4. encode_mfn_mem_kernel<.., ZC = true>: the memory recurrence per (case, row), then last_to_zy_fc1 with h_c the zero
//      row's last h -> zy_c;
//   5. the back end of zeros.hip: decode_factors_kernel with decoder c on (zy_c, z_c^0) and the classifier -> y_hat_c,
//      fc1_sqerr_kernel against the REAL x_c, zeros_finish_kernel (fp64, a fixed order, the counts of the WHOLE split).
// No float atomics: the results are bit-identical from run to run for a given (T, N, max_rows); a row's arithmetic does not
// depend on its place in a tile or a chunk, so y_hat is bit-identical for every chunking within one tile-row form.  Launch 2
// follows the launch rules of infer_dev.h: the per-block switch for the canonical size tuple only, else one launch per LSTM.
// The host side of launches 1, 3 and 4, the size parser, the refusals and the workspace parts behind the projections are the
// shared ones of encode_mfn_dev.h (its file head lists them); here: launch 2 with its one-row recurrences and the back end.
#include "encode_mfn_dev.h"

namespace mfm {

#define ZMFN_LSTMS 9          // the MFN's lstm l, a, v on x; the same three on zero input; encoder l, a, v on zero input

struct ZmfnOne {
  SeqDev seq;                                  // gates (read only), w_hh, h, Hp, hk4; an MFN LSTM: cs [T, n, Hp]
  const float* w[2]; const float* b[2];        // an encoder: fc1, the mean head
  float* z;                                    // an encoder: [rep, h], every row the one result
  float* h_last;                               // an MFN LSTM: its rows' last hidden states [n, h]
  int n, rep, nl, slot, block_begin;           // n: rows of this LSTM (1 on zero input); nl: 2 with the mean head, else 1;
};                                             // slot: which of K0 .. K5 is its size (MFN l, a, v, encoder l, a, v)
struct ZmfnSeqDev { ZmfnOne d[ZMFN_LSTMS]; int count, T, maxw; };

// ENC0: slot 0 is an encoder's size (the launches of one LSTM each); slots 3 .. 5 always are
template <int R, bool ENC0, int K0, int K1, int K2, int K3, int K4, int K5>
__global__ __launch_bounds__(1024) void zeros_mfn_seq_kernel(const ZmfnSeqDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, bid = blockIdx.x;
  MFM_SEQ_BLOCK_LSTM(P, bid, li)
  const ZmfnOne& E = P.d[li];
  const int di = E.slot;
  const int tile = bid - E.block_begin, b0 = tile * R;
  const int h = E.seq.h;
  const float* hT = nullptr;
  if (di < 3 && !(ENC0 && di == 0)) {
    if constexpr (!ENC0) { MFM_TUPLE_ONE(0, K0, (hT = small_fwd_body<KQ, R, false, false, false, false, true>(E.seq, P.T, E.n, tile, lds))) }
    MFM_TUPLE_ONE(1, K1, (hT = small_fwd_body<KQ, R, false, false, false, false, true>(E.seq, P.T, E.n, tile, lds)))
    MFM_TUPLE_ONE(2, K2, (hT = small_fwd_body<KQ, R, false, false, false, false, true>(E.seq, P.T, E.n, tile, lds)))
    store_rows<R>(hT, E.h_last, h, b0, E.n, tid);
    return;
  }
  if constexpr (ENC0) { MFM_TUPLE_ONE(0, K0, (hT = small_fwd_body<KQ, R, false, false, false>(E.seq, P.T, E.n, tile, lds))) }
  MFM_TUPLE_ONE(3, K3, (hT = small_fwd_body<KQ, R, false, false, false>(E.seq, P.T, E.n, tile, lds)))
  MFM_TUPLE_ONE(4, K4, (hT = small_fwd_body<KQ, R, false, false, false>(E.seq, P.T, E.n, tile, lds)))
  MFM_TUPLE_ONE(5, K5, (hT = small_fwd_body<KQ, R, false, false, false>(E.seq, P.T, E.n, tile, lds)))
  // the two h buffers stay where they are; fc1's output and the head's behind them ([maxw][R] each)
  float* act0 = lds + 2 * E.seq.Hp * R;
  float* act1 = act0 + P.maxw * R;
  dense_rows<R>(E.w[0], E.b[0], h, h, hT, act0, false);
  const float* zr = act0;
  if (E.nl == 2) {
    dense_rows<R>(E.w[1], E.b[1], h, h, act0, act1, false);
    zr = act1;
  }
  for (int e = tid; e < E.rep * h; e += blockDim.x) E.z[e] = zr[(e % h) * R];
}

// the constant gates cg[i] [T, 4, Hp[i]] of the six one-row recurrences: b_ih + b_hh at every step, pad units u >= h exact zeros
struct ZmfnGatesDev { float* cg[6]; const float* b_ih[6]; const float* b_hh[6]; int h[6], Hp[6], T; };

__global__ __launch_bounds__(256) void zeros_mfn_cgates_kernel(const ZmfnGatesDev G) {
  const int gtid = blockIdx.x * blockDim.x + threadIdx.x, gstride = gridDim.x * blockDim.x;
#pragma unroll 1
  for (int m = 0; m < 6; ++m) {
    const int h = G.h[m], Hp = G.Hp[m];
    for (int i = gtid; i < G.T * 4 * Hp; i += gstride) {
      const int u = i % Hp, g = (i / Hp) & 3;
      G.cg[m][i] = (u < h) ? G.b_ih[m][g * h + u] + G.b_hh[m][g * h + u] : 0.0f;
    }
  }
}

// ---------------------------------------------------------------- host
static const int kZmfnCanon[6] = {22, 16, 12, 8, 2, 20};      // the MFN's LSTMs h = 88 / 64 / 48, encoders h = 32 / 8 / 80

// the workspace, in this order (every part a multiple of 4 floats; include/mfm_hip.h states it term by term): the chunk's three
// x-projections and, behind the recurrences, the decoders' h in the same place; the parts of mfn_ws, the chain's buffers for the 3
// rows T triples; the six constant gate sets; the one-row c records and last hidden states; the zeroed encoders' factors, one row
// per chunk row; zy of the three cases; the squared-error partials; the fp64 accumulators
struct ZmfnLayout { int64_t cg[6], cz[3], hz[3], zc[3], o_cs, o_zy, o_part, o_acc, total; };
static ZmfnLayout zmfn_layout(const MfnSizes& Z, int64_t T, int64_t N, int64_t max_rows) {
  const EmfnSizes& S = Z.E;
  const int64_t rows = gen_rows(N, max_rows);
  ZmfnLayout L;
  int64_t g = 0;
  for (int m = 0; m < 3; ++m) g += rows * T * 4 * hp_of(S.hm[m]);
  L.o_cs = std::max(g, decode_ws_floats(T, N, Z.dec[7], Z.dec[4], Z.dec[5], Z.dec[6], max_rows));
  int64_t o = L.o_cs + mfn_ws(S, T, rows, 3).total;
  for (int i = 0; i < 6; ++i) { L.cg[i] = T * 4 * hp_of(i < 3 ? S.hm[i] : S.z[i - 3]); o += L.cg[i]; }
  for (int m = 0; m < 3; ++m) { L.cz[m] = T * hp_of(S.hm[m]); L.hz[m] = up4(S.hm[m]); L.zc[m] = up4(rows * S.z[m]); o += L.cz[m] + L.hz[m] + L.zc[m]; }
  L.o_zy = o;
  L.o_part = L.o_zy + up4(3 * rows * S.zy);
  L.o_acc = L.o_part + up4(fc1_sqerr_tiles(T, rows, Z.dec + 8));
  L.total = L.o_acc + up4(2 * ZER_ACC);
  return L;
}

// the launch(es) of the recurrences of one chunk: P.d[0 .. P.count) filled but for block_begin.  canon: all six sizes are the
// canonical ones (every chunk of a call takes the same kernels, whichever LSTMs it runs)
template <int R>
static int zmfn_seq_launch(const char* who, ZmfnSeqDev& P, bool canon, int threads, size_t lds_bytes, hipStream_t stream) {
  static const char* name = "zeros_mfn_seq_kernel";
  if (canon) {
    int blocks = 0;
    for (int i = 0; i < P.count; ++i) {
      P.d[i].block_begin = blocks;
      blocks += cdiv(P.d[i].n, R);
    }
    return seq_launch_kernel(zeros_mfn_seq_kernel<R, false, 22, 16, 12, 8, 2, 20>, name, dim3(blocks), dim3(threads), lds_bytes, stream, nullptr, P);
  }
  // other sizes: one launch per LSTM of the kernel instantiated for its size alone (the launch rules of infer_dev.h)
  for (int i = 0; i < P.count; ++i) {
    ZmfnSeqDev Q = P;
    const bool enc = P.d[i].slot >= 3;
    Q.d[0] = P.d[i]; Q.d[0].block_begin = 0; Q.d[0].slot = 0; Q.count = 1;
    const int tiles = cdiv(Q.d[0].n, R), th = std::max(8 * Q.d[0].seq.Hp, 64);
    const int rc = enc
      ? infer_launch_hk4(who, name, Q.d[0].seq, [](auto kk) { return zeros_mfn_seq_kernel<R, true, decltype(kk)::value, 0, 0, 0, 0, 0>; }, Q, tiles, th, lds_bytes, stream)
      : infer_launch_hk4(who, name, Q.d[0].seq, [](auto kk) { return zeros_mfn_seq_kernel<R, false, decltype(kk)::value, 0, 0, 0, 0, 0>; }, Q, tiles, th, lds_bytes, stream);
    if (rc != MFM_OK) return rc;
  }
  return MFM_OK;
}

static int predict_zeros_mfn(int T, int64_t N, const int32_t* sz, const float* params, const int64_t* offs, const float* x,
                             const void* y, float* ws, float* y_hat, float* gen, float* disc, int64_t max_rows, hipStream_t stream) {
  static const char* who = "predict zeros mfn";
  MfnSizes Z;
  MFM_REQUIRE(T >= 1 && N >= 1 && mfn_sizes(sz, Z),
              "%s: sizes must be positive (T %d, N %lld, and the %d sizes; heads and the loss kind 0 or 1)", who, T, (long long)N, MFN_SIZES);
  MFM_REQUIRE(params && offs && x && ws && y_hat && gen,
              "%s: bad arguments (params, offsets, x, workspace, y_hat and gen must not be null)", who);
  MFM_REQUIRE((y != nullptr) == (disc != nullptr), "%s: labels and disc come together (both, or both null)", who);
  const EmfnSizes& S = Z.E;
  int rc = infer_check_aligned(who, params, x, ws);
  if (rc != MFM_OK) return rc;
  if ((rc = infer_check_rows(who, N, max_rows)) != MFM_OK) return rc;
  // the offsets of mfm_encode_mfn, then the 38 of mfm_decode_factors (decode_factors_prepare checks those)
  const int EO = S.heads ? 10 : 6, o_mfn = 3 * EO, o_att = o_mfn + 12, o_zy = o_att + 16, o_dec = o_zy + (S.heads ? 4 : 2);
  if ((rc = infer_check_offsets(who, offs, o_mfn, EO)) != MFM_OK) return rc;
  if ((rc = infer_check_offsets(who, offs + o_mfn, o_dec - o_mfn, 4, 0, 12)) != MFM_OK) return rc;
  if ((rc = mfn_check_covered(who, S, true)) != MFM_OK) return rc;
  const int D = S.d[0] + S.d[1] + S.d[2], od = Z.od, loss_kind = Z.loss_kind;
  const int rows = (int)gen_rows(N, max_rows);
  const int R = gen_tile_rows(3, rows);
  int maxw = 1, hmax = 1, threads = 64;
  size_t seq_floats = 0;
  for (int i = 0; i < 3; ++i) {
    maxw = std::max(maxw, S.z[i]);
    hmax = std::max(hmax, std::max(S.z[i], S.hm[i]));
  }
  threads = std::max(threads, 8 * round_up(hmax, 16));
  for (int i = 0; i < 3; ++i)
    seq_floats = std::max(seq_floats, std::max(seq_lds_floats(S.hm[i], R), enc_lds_floats(S.z[i], R, 2, maxw)));
  const size_t seq_lds = lds_bytes_of(seq_floats);
  if ((rc = infer_check_lds(who, seq_lds, hmax, R)) != MFM_OK) return rc;
  EmfnChain C;
  if ((rc = emfn_chain_check(who, S, 3 * (int64_t)T * rows, C)) != MFM_OK) return rc;
  // (the chain's buffers hold 3 rows per chunk row)
  if ((rc = infer_check_chunk(who, rows, T, std::max(std::max(D, 4 * round_up(hmax, 16)), 3 * std::max(S.M, std::max(S.H1, S.H2))), "projection")) != MFM_OK)
    return rc;
  DecLaunch Dl;
  Fc1SqLaunch Sq;
  if ((rc = decode_factors_prepare(who, T, N, Z.dec, params, offs + o_dec, ws, max_rows, Dl)) != MFM_OK) return rc;
  if ((rc = fc1_sqerr_prepare(who, Dl, N, Sq)) != MFM_OK) return rc;

  // ---- everything that does not depend on the chunk
  const ZmfnLayout lay = zmfn_layout(Z, T, N, max_rows);
  ZmfnSeqDev P;
  ZmfnGatesDev G;
  memset(&P, 0, sizeof(P));
  memset(&G, 0, sizeof(G));
  EmfnAttDev& A = C.A;
  EmfnMemDev& Mm = C.Mm;
  emfn_chain_fill(C, S, T, params, offs + o_att, offs + o_zy, 1);
  MfnLstm L[3];
  float* zc[3];
  {
    for (int m = 0; m < 3; ++m) {          // the MFN's LSTMs on x; the chain's buffers hold the 3 cases
      L[m] = MfnLstm{&P.d[m].seq, &P.d[m].h_last, 0, 0};
      P.d[m].slot = m;
    }
    float* w0 = mfn_lstms_fill(L, C, S, T, rows, 3, params, offs + o_mfn, ws, ws + lay.o_cs);
    for (int i = 0; i < 6; ++i) {          // the six one-row recurrences: the MFN's LSTMs, then the encoders, on zero input
      ZmfnOne& E = P.d[3 + i];
      const int m = i % 3;
      const int64_t* o = i < 3 ? offs + o_mfn + 4 * m : offs + EO * m;
      seq_fill(E.seq, params + o[0], params + o[1], params + o[2], params + o[3], i < 3 ? S.hm[m] : S.z[m], 0);
      E.seq.gates = w0;
      G.cg[i] = w0; G.b_ih[i] = params + o[2]; G.b_hh[i] = params + o[3]; G.h[i] = E.seq.h; G.Hp[i] = E.seq.Hp;
      w0 += lay.cg[i];
      E.n = 1; E.slot = i;
      if (i >= 3) {
        E.nl = S.heads ? 2 : 1;
        for (int l = 0; l < E.nl; ++l) { E.w[l] = params + o[4 + 2 * l]; E.b[l] = params + o[5 + 2 * l]; }
        E.rep = rows;
      }
    }
    G.T = T;
    for (int m = 0; m < 3; ++m) {
      P.d[3 + m].seq.cs = w0; A.cz[m] = w0; w0 += lay.cz[m];
      P.d[3 + m].h_last = w0; Mm.hz[m] = w0; w0 += lay.hz[m];
      P.d[6 + m].z = zc[m] = w0; w0 += lay.zc[m];
    }
  }
  P.T = T; P.maxw = maxw;
  bool canon = true;
  for (int i = 0; i < ZMFN_LSTMS; ++i) canon = canon && P.d[i].seq.hk4 == kZmfnCanon[P.d[i].slot];
  float* zyb = ws + lay.o_zy;                                     // [3, n, zy] of the chunk
  float* part = ws + lay.o_part;
  double* acc = reinterpret_cast<double*>(ws + lay.o_acc);      // (a multiple of 4 floats from a 16-byte aligned base)
  Mm.oz[0] = zyb;

  ZerFinishDev Q;
  memset(&Q, 0, sizeof(Q));
  for (int m = 0; m < ZER_CASES; ++m) Q.inv_gen[m] = Sq.inv_gen[m];
  Q.acc = acc; Q.gen = gen; Q.disc = disc;
  Q.inv_disc = inv_label_count(loss_kind, N, od);
  Q.od = od; Q.loss_kind = loss_kind;

  for (int64_t n0 = 0; n0 < N; n0 += rows) {
    const int n = (int)std::min<int64_t>(rows, N - n0);
    const bool first = n0 == 0;
    rc = mfn_xproj_chunk(3, L, x, T, N, D, n0, n, stream);
    if (rc != MFM_OK) return rc;
    if (first) {
      zeros_mfn_cgates_kernel<<<dim3(8), dim3(256), 0, stream>>>(G);
      MFM_LAUNCH_CHECK("zeros_mfn_cgates_kernel");
    }
    for (int m = 0; m < 3; ++m) P.d[m].n = n;
    P.count = first ? ZMFN_LSTMS : 3;      // the one-row results do not depend on the chunk: the first one computes them
    rc = (R == 1) ? zmfn_seq_launch<1>(who, P, canon, threads, seq_lds, stream) : zmfn_seq_launch<4>(who, P, canon, threads, seq_lds, stream);
    if (rc != MFM_OK) return rc;
    if ((rc = emfn_chain_launch<true>(C, T, n, stream)) != MFM_OK) return rc;
    // (the projections are dead behind the recurrences: the decoders' h takes their place)
    DecodeDev& PD = Dl.P;
    PD.n = n;
    for (int c = 0; c < ZER_CASES; ++c) {
      PD.d[c].zm = zc[c]; PD.d[c].zy = zyb + (int64_t)c * n * S.zy;
      PD.d[c].y_hat = y_hat + ((int64_t)c * N + n0) * od;
    }
    if ((rc = decode_factors_launch(who, PD, Dl.R, Dl.threads, Dl.lds_bytes, stream)) != MFM_OK) return rc;
    if ((rc = fc1_sqerr_chunk(Sq, x, n0, n, part, Q.part, Q.npart, stream)) != MFM_OK) return rc;
    for (int c = 0; c < ZER_CASES; ++c) Q.y_hat[c] = PD.d[c].y_hat;
    Q.y = labels_at(y, loss_kind, n0, od);
    Q.n = n; Q.first = first; Q.last = n0 + n == N;
    if ((rc = zeros_finish_launch(Q, stream)) != MFM_OK) return rc;
  }
  return MFM_OK;
}

}  // namespace mfm

extern "C" int64_t mfm_predict_zeros_mfn_workspace_floats(int32_t T, int64_t N, const int32_t* sizes, int64_t max_rows) {
  mfm::MfnSizes Z;
  if (T < 1 || N < 1 || max_rows < 0 || !sizes || !mfm::mfn_sizes(sizes, Z)) return 0;
  return mfm::zmfn_layout(Z, T, N, max_rows).total;
}

extern "C" int mfm_predict_zeros_mfn_tile_rows(int64_t N, int64_t max_rows) {
  if (N < 1 || max_rows < 0) return -1;
  return mfm::gen_tile_rows(3, (int)mfm::gen_rows(N, max_rows));
}

extern "C" int mfm_predict_zeros_mfn(int32_t T, int64_t N, const int32_t* sizes, const float* params, const int64_t* offsets,
                                     const float* x, const void* y, float* workspace, float* y_hat, float* gen, float* disc,
                                     int64_t max_rows, void* stream) {
  return mfm::predict_zeros_mfn(T, N, sizes, params, offsets, x, y, workspace, y_hat, gen, disc, max_rows, (hipStream_t)stream);
}
