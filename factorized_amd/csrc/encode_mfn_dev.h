// The Memory Fusion Network behind the MFN LSTMs, shared by the four no-plan entries of MFM_KL and MFM (encode_mfn.hip,
// objective_mfn.hip, zeros_mfn.hip, predict_mfn.hip): the attention chain (encode_mfn_att_kernel) and the memory recurrence with
// the label head (encode_mfn_mem_kernel), the size arrays they are described by and the host side the entries have in common.
// Template parameter ZC of both kernels: false, the rows of the chain are the chunk's n rows; true, they are the 3 n (case c, row
// i) of the zeroed-modality protocol, case major (mfm_predict_zeros_mfn): modality c's cell states and last hidden state come from
// the ONE row the MFN's LSTM c computes on zero input (cz / hz), the other two modalities' from the real records.  Only the gather
// differs; the arithmetic of a row is the same code.  zeros_mfn.hip alone instantiates ZC = true.
// Template parameter TAIL of the memory recurrence (off by default; predict_mfn.hip and ablation_mfn.hip turn it on, with ZC =
// false): zy stays in LDS and the same workgroup goes on with zy_to_fy and the classifier, writes the row of y_hat and, with
// labels, the row's loss contribution (EmfnTailDev); the other instantiations do not see any of it.  EMB (with TAIL;
// ablation_mfn.hip alone): the workgroup also stores the row's fy, which it holds in LDS behind zy_to_fy_fc2, for the decoders.
// Host, shared by all four (and by ablation_mfn.hip, whose parameters are separate tensors: the *_ptrs forms): the two size parsers (emfn_sizes, the 17 of mfm_encode_mfn; mfn_sizes, the MFN_SIZES of the other
// three), the refusals (mfn_check_covered), the sizing of the two launches (emfn_chain_check / emfn_chain_fill) and the launches
// themselves (emfn_att_launch, emfn_mem_launch, emfn_chain_launch), the workspace parts behind the x-projections (mfn_ws), the
// MFN's three LSTMs of a call (mfn_lstms_fill); a chunk's grouped projection GEMM (MfnLstm, mfn_xproj_chunk) is in infer_dev.h,
// where ablation.hip drives it too.
// At the end of the file: the launch in front of the chain as mfm_encode_mfn runs it -- the six recurrences (encoder l, a, v with
// their heads, the MFN's LSTMs with their cell-state records) in one launch, encode_mfn_seq_kernel, its workspace parts and its
// launcher; encode_mfn_front.h walks them chunk by chunk for mfm_encode_mfn and mfm_objective_mfn.  Nothing above that section
// names it: zeros_mfn.hip and predict_mfn.hip include this header and must not instantiate that kernel.
#pragma once
#include "infer_dev.h"

namespace mfm {

#define EMFN_LSTMS 6          // encoder l, a, v, then the MFN's lstm l, a, v
#define EMFN_SIZES 17
#define MFN_SIZES 23          // the sizes of the entries with a back end: the 17, then fl, fa, fv, fy, output_dim, the loss kind
#define EMFN_ATT_THREADS 512
#define EMFN_SPARTS 16        // threads per pair in the softmax: fixed, the sums' order must not depend on the tile width
#define EMFN_MAXW 32          // weights per thread and matrix of the memory recurrence

// ---------------------------------------------------------------- the attention chain
struct EmfnAttDev {
  const float* cs[3];                          // the MFN LSTMs' c records [T, n, Hp]
  const float* cz[3];                          // ZC: the one-row c records [T, 1, Hp] of the MFN LSTMs on zero input
  const float* w[6]; const float* b[6];        // att1_fc1, att1_fc2, att2_fc1, att2_fc2, gamma1_fc1, gamma2_fc1
  float* chat; float* g1p; float* g2p;         // [T nv, M], [T nv, H1], [T nv, H2]; nv = n (ZC: 3 n) rows of the chain
  int hm[3], Hpm[3];
  int T, n, tot, KC, KCp, h1, h2, hbp, M, H1, H2;
};

// Y[o][pair] = sum_k W[o][k] X[k][pair] over the tile's 16 CT pairs: wave w takes the 16-unit output tiles w, w + waves, ...;
// X in LDS as [Kp][LDP] (rows K .. Kp exact zeros), LDP = 16 CT + 4 (the four k a B fragment reads fall on different banks).
// MFMA step s of chunk c multiplies k = 16 c + 4 (lane >> 4) + s on both sides: a lane's four A values are one 16-byte load of
// its weight row (K and the row stride multiples of 4 and an aligned base; else four guarded dword loads), the next chunk's
// while this one multiplies.  Rows beyond Nout and columns beyond K read as zeros.  epi(o, pair, value) for the lane's
// 4 x CT results: o = 16 tile + 4 (lane >> 4) + r, pair = 16 ct + (lane & 15)
template <int CT, class Epi>
__device__ __forceinline__ void emfn_layer(const float* __restrict__ W, const int ldw, const int K, const int Kp, const int Nout,
                                           const int out_tiles, const float* Xs, Epi epi) {
  constexpr int LDP = 16 * CT + 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int col = lane & 15, q = lane >> 4;
  const bool vec = (ldw & 3) == 0 && (K & 3) == 0 && (((uintptr_t)W) & 15) == 0;
  const int kchunks = Kp / 16;
  for (int ot = wave; ot < out_tiles; ot += nw) {
    const int orow = 16 * ot + col;
    const bool rok = orow < Nout;
    const float* wr = W + (int64_t)min(orow, Nout - 1) * ldw;
    auto lda = [&](const int c) {
      const int k0 = 16 * c + 4 * q;
      f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
      if (vec) {
        if (rok && k0 < K) v = *reinterpret_cast<const f32x4*>(wr + k0);
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (rok && k0 + i < K) v[i] = wr[k0 + i];
      }
      return v;
    };
    f32x4 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 a4 = lda(0);
    for (int c = 0; c < kchunks; ++c) {
      const f32x4 an = lda(c + 1 < kchunks ? c + 1 : c);
      const float* bc = Xs + (16 * c + 4 * q) * LDP + col;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[ct] = mma16x16x4(a4[s], bc[s * LDP + 16 * ct], acc[ct]);
      }
      a4 = an;
    }
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) epi(16 * ot + 4 * q + r, 16 * ct + col, acc[ct][r]);
  }
}

template <int CT, bool ZC>
__global__ __launch_bounds__(EMFN_ATT_THREADS) void encode_mfn_att_kernel(const EmfnAttDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int MT = 16 * CT, LDP = MT + 4;
  const int tid = threadIdx.x;
  const int KC = P.KC, KCp = P.KCp, tot = P.tot;
  const int64_t pairs = (int64_t)P.T * (ZC ? 3 : 1) * P.n, p0 = (int64_t)blockIdx.x * MT;
  float* Xc = lds;                             // [KCp][LDP] cStar
  float* Lg = Xc + KCp * LDP;                  // [KCp][LDP] the attention's logits, then attended
  float* Hb = Lg + KCp * LDP;                  // [hbp][LDP] the hidden layer of att1, then of att2
  float* red = Hb + P.hbp * LDP;               // [2][EMFN_SPARTS][MT]

  // ---- cStar of the tile's pairs: k < tot from step t - 1 (zeros at t = 0), the rest from step t; unit fastest
  const int n0 = P.hm[0], n1 = n0 + P.hm[1];
  for (int e = tid; e < KCp * MT; e += EMFN_ATT_THREADS) {
    const int j = e / KCp, k = e - j * KCp;
    const int64_t p = p0 + j;
    float v = 0.0f;
    if (k < KC && p < pairs) {
      const int prev = k < tot, u = prev ? k : k - tot;
      const int m = u < n0 ? 0 : (u < n1 ? 1 : 2);
      const int um = u - (m == 0 ? 0 : (m == 1 ? n0 : n1));
      if constexpr (ZC) {
        // pair p = (t, case c, row i): the zeroed modality's columns from its one-row record, the same for every row
        const int nv = 3 * P.n;
        const int t = (int)(p / nv), r = (int)(p - (int64_t)t * nv);
        const int c = r / P.n, i = r - c * P.n;
        if (!prev || t > 0)
          v = (m == c) ? P.cz[m][(int64_t)(t - prev) * P.Hpm[m] + um] : P.cs[m][((int64_t)(t - prev) * P.n + i) * P.Hpm[m] + um];
      } else {
        const int t = (int)(p / P.n), i = (int)(p - (int64_t)t * P.n);
        if (!prev || t > 0) v = P.cs[m][((int64_t)(t - prev) * P.n + i) * P.Hpm[m] + um];
      }
    }
    Xc[k * LDP + j] = v;
  }
  lds_barrier();

  // ---- att1: hidden = relu(fc1 cStar), logits = fc2 hidden
  emfn_layer<CT>(P.w[0], KC, KC, KCp, P.h1, P.hbp / 16, Xc, [&](const int o, const int j, const float v) {
    Hb[o * LDP + j] = o < P.h1 ? fmaxf(v + P.b[0][o], 0.0f) : 0.0f;
  });
  lds_barrier();
  emfn_layer<CT>(P.w[1], P.h1, P.h1, (P.h1 + 15) / 16 * 16, KC, KCp / 16, Hb, [&](const int o, const int j, const float v) {
    Lg[o * LDP + j] = o < KC ? v + P.b[1][o] : 0.0f;
  });
  lds_barrier();

  // ---- attended = softmax(logits) * cStar per pair: EMFN_SPARTS threads per pair, every sum in a fixed order
  {
    const int j = tid % MT, part = tid / MT;
    const bool on = tid < EMFN_SPARTS * MT;
    float mx = -INFINITY;
    if (on)
      for (int k = part; k < KC; k += EMFN_SPARTS) mx = fmaxf(mx, Lg[k * LDP + j]);
    if (on) red[part * MT + j] = mx;
    lds_barrier();
    if (on) {
#pragma unroll
      for (int s = 0; s < EMFN_SPARTS; ++s) mx = fmaxf(mx, red[s * MT + j]);
    }
    float sum = 0.0f;
    if (on)
      for (int k = part; k < KC; k += EMFN_SPARTS) {
        const float ev = expf(Lg[k * LDP + j] - mx);
        Lg[k * LDP + j] = ev;
        sum += ev;
      }
    float* red2 = red + EMFN_SPARTS * MT;
    if (on) red2[part * MT + j] = sum;
    lds_barrier();
    if (on) {
      float tsum = red2[j];
#pragma unroll
      for (int s = 1; s < EMFN_SPARTS; ++s) tsum += red2[s * MT + j];
      for (int k = part; k < KC; k += EMFN_SPARTS) Lg[k * LDP + j] = Lg[k * LDP + j] / tsum * Xc[k * LDP + j];
    }
  }
  lds_barrier();

  // ---- att2: cHat = tanh(fc2 relu(fc1 attended))
  emfn_layer<CT>(P.w[2], KC, KC, KCp, P.h2, P.hbp / 16, Lg, [&](const int o, const int j, const float v) {
    Hb[o * LDP + j] = o < P.h2 ? fmaxf(v + P.b[2][o], 0.0f) : 0.0f;
  });
  lds_barrier();
  emfn_layer<CT>(P.w[3], P.h2, P.h2, (P.h2 + 15) / 16 * 16, P.M, (P.M + 15) / 16, Hb, [&](const int o, const int j, const float v) {
    if (o < P.M && p0 + j < pairs) P.chat[(p0 + j) * P.M + o] = tanhf(v + P.b[3][o]);
  });
  // ---- the attended columns of gamma1_fc1 / gamma2_fc1 (their rows are KC + M wide), with the bias
  emfn_layer<CT>(P.w[4], KC + P.M, KC, KCp, P.H1, (P.H1 + 15) / 16, Lg, [&](const int o, const int j, const float v) {
    if (o < P.H1 && p0 + j < pairs) P.g1p[(p0 + j) * P.H1 + o] = v + P.b[4][o];
  });
  emfn_layer<CT>(P.w[5], KC + P.M, KC, KCp, P.H2, (P.H2 + 15) / 16, Lg, [&](const int o, const int j, const float v) {
    if (o < P.H2 && p0 + j < pairs) P.g2p[(p0 + j) * P.H2 + o] = v + P.b[5][o];
  });
}

// ---------------------------------------------------------------- the memory recurrence and the label head
struct EmfnMemDev {
  const float* g1p; const float* g2p; const float* chat;      // [T, n, H1], [T, n, H2], [T, n, M]
  const float* w1m; const float* w2m;                          // the memory columns of gamma*_fc1, rows ldw apart
  const float* w1b; const float* b1b; const float* w2b; const float* b2b;      // gamma*_fc2
  const float* hl[3];                                          // the MFN LSTMs' last hidden states [n, h_m] (ZC: [nreal, h_m])
  const float* hz[3];                                          // ZC: the last hidden state [h_m] of MFN LSTM m on zero input
  const float* wz[2]; const float* bz[2]; float* oz[2];        // last_to_zy_fc1, last_to_logvarzy_fc1; the chunk's rows [n, zy]
  int hn[3];
  int T, n, M, H1, H2, QA, QB, MP, HP, ldw, tot, zy, nheads;   // n: the rows of the recurrence (ZC: 3 nreal, case major)
  int nreal;                                                   // ZC: the chunk's rows
};
// all-reduce over groups of Q adjacent lanes, Q in {1, 2, 4, 8, 16}
__device__ __forceinline__ float emfn_group_sum(float v, const int Q) {
  if (Q >= 2) v += dpp_f<DPP_QUAD_XOR1>(v);
  if (Q >= 4) v += dpp_f<DPP_QUAD_XOR2>(v);
  if (Q >= 8) v += dpp_f<DPP_ROW_HALF_MIRROR>(v);
  if (Q >= 16) v += dpp_f<DPP_ROW_MIRROR>(v);
  return v;
}

// a thread's resident weights: elements [k0, k0 + 32) of one weight row, zeros beyond n; whole aligned slices as 16-byte loads
__device__ __forceinline__ void emfn_wslice(float (&w)[EMFN_MAXW], const float* __restrict__ row, const int k0, const int n, const bool act) {
  const float* src = row + k0;
  if (act && k0 + EMFN_MAXW <= n && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
#pragma unroll
    for (int i = 0; i < EMFN_MAXW / 4; ++i) {
      const f32x4 v = reinterpret_cast<const f32x4*>(src)[i];
      w[4 * i] = v[0]; w[4 * i + 1] = v[1]; w[4 * i + 2] = v[2]; w[4 * i + 3] = v[3];
    }
  } else {
#pragma unroll
    for (int i = 0; i < EMFN_MAXW; ++i) w[i] = (act && k0 + i < n) ? row[min(k0 + i, n - 1)] : 0.0f;
  }
}

// TAIL: what the label tail behind the recurrence adds (mfm_predict_mfn); wz[0] / bz[0] are read, oz is not
struct EmfnTailDev : EmfnMemDev {
  const float* wt[4]; const float* bt[4];      // zy_to_fy_fc1, zy_to_fy_fc2, fy_to_y_fc1, fy_to_y_fc2
  const void* y; float* y_hat;                 // this chunk's labels (null: no loss) and outputs [n, od]
  float* rowloss; double* acc; int* ticket;    // workspace: one contribution per row of the chunk, the running sum, the ticket word
  float* loss;                                 // the result (null: no loss)
  double inv;                                  // 1 / (N od) (L1) or 1 / N (CE) over the WHOLE split
  int fy, od, loss_kind, tailw, first, last;   // tailw: floats of one tail activation in LDS; first / last chunk of the call
  float* emb; int embw;                        // EMB: the chunk's embedding block [n, embw]; the row's fy goes to its columns [0, fy)
};

// one layer of the tail on LDS vectors, 8 lanes per output as the head: out[o] = (relu)(b[o] + sum_k W[o][k] in[k])
__device__ __forceinline__ void emfn_tail_layer(const float* __restrict__ W, const float* __restrict__ b, const int K, const int Nout,
                                                const float* in, float* out, const bool relu, const int tid) {
  const int q8 = tid & 7;
  for (int o = tid >> 3; o < Nout; o += (int)blockDim.x >> 3) {
    const float* wr = W + (int64_t)o * K;
    float s = 0.0f;
    for (int k = q8; k < K; k += 8) s = fmaf(wr[k], in[k], s);
    s = emfn_group_sum(s, 8) + b[o];
    if (q8 == 0) out[o] = relu ? fmaxf(s, 0.0f) : s;
  }
  lds_barrier();
}

// The thread roles, the operand layout (lane q of a group owns the contiguous slice [32 q, 32 q + 32) of the reduction) and the
// two barriers per step are those of mfn_mem_fwd_kernel (mfn_mem.hip); nothing of a step is stored
template <int MAXT, bool ZC, bool TAIL = false, bool EMB = false>
__global__ __launch_bounds__(MAXT) void encode_mfn_mem_kernel(const std::conditional_t<TAIL, EmfnTailDev, EmfnMemDev> P) {
  static_assert(!(TAIL && ZC), "the label tail runs on the chunk's own rows");
  static_assert(!EMB || TAIL, "fy exists in the label tail alone");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int T = P.T, n = P.n, M = P.M, H1 = P.H1, H2 = P.H2, QA = P.QA, QB = P.QB, MP = P.MP, HP = P.HP;
  float* memb = lds;                 // [2][MP]
  float* ab = lds + 2 * MP;          // [2][HP] the relu activations of the two gates
  const int row = blockIdx.x, tid = threadIdx.x;

  // phase A: (gate, j, q): u[j] = relu(partial[t][j] + sum_k Wm[j][k] mem[k])
  const int nA = (H1 + H2) * QA;
  const bool actA = tid < nA;
  const int ja = min(tid, nA - 1) / QA, qa = tid % QA;
  const int netA = ja >= H1;
  const int jn = netA ? ja - H1 : ja;
  const int Hn = netA ? H2 : H1;
  float wA[EMFN_MAXW];
  emfn_wslice(wA, (netA ? P.w2m : P.w1m) + (int64_t)jn * P.ldw, EMFN_MAXW * qa, M, actA);
  const float* abuf = netA ? P.g2p : P.g1p;
  // phase B: (m, q): gamma_g[m] = sigmoid(b[m] + sum_k Wb_g[m][k] u_g[k]), both gates
  const int nB = M * QB;
  const bool actB = tid < nB;
  const int mb = min(tid, nB - 1) / QB, qb = tid % QB;
  float wB1[EMFN_MAXW], wB2[EMFN_MAXW];
  emfn_wslice(wB1, P.w1b + (int64_t)mb * H1, EMFN_MAXW * qb, H1, actB);
  emfn_wslice(wB2, P.w2b + (int64_t)mb * H2, EMFN_MAXW * qb, H2, actB);
  const float bb1 = P.b1b[mb], bb2 = P.b2b[mb];

  for (int i = tid; i < 2 * MP + 2 * HP; i += blockDim.x) lds[i] = 0.0f;
  float memr = 0.0f;                              // mem[mb], the same in every lane of the phase-B group
  const int64_t arow = (int64_t)row * Hn + jn, mrow = (int64_t)row * M + mb;
  float att_n = abuf[arow], ch_n = P.chat[mrow];
  lds_barrier();
  const bool stA = actA && qa == 0, stB = actB && qb == 0;
  int cur = 0;
  for (int t = 0; t < T; ++t) {
    const float att = att_n, ch = ch_n;
    const int tn = min(t + 1, T - 1);
    att_n = abuf[(int64_t)tn * n * Hn + arow];     // unconditional prefetch (clamped at the tail)
    ch_n = P.chat[(int64_t)tn * n * M + mrow];
    {
      const f32x4* mp = reinterpret_cast<const f32x4*>(memb + cur * MP + EMFN_MAXW * qa);
      float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
      for (int i = 0; i < EMFN_MAXW / 4; ++i) {
        const f32x4 v = mp[i];
        s0 = fmaf(wA[4 * i], v[0], s0); s1 = fmaf(wA[4 * i + 1], v[1], s1);
        s0 = fmaf(wA[4 * i + 2], v[2], s0); s1 = fmaf(wA[4 * i + 3], v[3], s1);
      }
      const float u = fmaxf(emfn_group_sum(s0 + s1, QA) + att, 0.0f);
      if (stA) ab[netA ? HP + jn : jn] = u;
    }
    lds_barrier();
    {
      const f32x4* a1p = reinterpret_cast<const f32x4*>(ab + EMFN_MAXW * qb);
      const f32x4* a2p = reinterpret_cast<const f32x4*>(ab + HP + EMFN_MAXW * qb);
      float z1 = 0.0f, z2 = 0.0f;
#pragma unroll
      for (int i = 0; i < EMFN_MAXW / 4; ++i) {
        const f32x4 v1 = a1p[i], v2 = a2p[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) { z1 = fmaf(wB1[4 * i + e], v1[e], z1); z2 = fmaf(wB2[4 * i + e], v2[e], z2); }
      }
      const float g1 = act_sigmoid(emfn_group_sum(z1, QB) + bb1), g2 = act_sigmoid(emfn_group_sum(z2, QB) + bb2);
      memr = g1 * memr + g2 * ch;
      if (stB) memb[(cur ^ 1) * MP + mb] = memr;
    }
    lds_barrier();
    cur ^= 1;
  }

  // ---- the heads on [h_l | h_a | h_v | mem_T]: the vector into LDS (over the recurrence's buffers, which nobody reads any
  // more), then 8 lanes per output
  const int KT = P.tot + M, nout = P.nheads * P.zy;
  float* vec = lds;
  const int m0 = P.hn[0], m1 = m0 + P.hn[1];
  for (int k = tid; k < P.tot; k += blockDim.x) {
    const int m = k < m0 ? 0 : (k < m1 ? 1 : 2);
    const int km = k - (m == 0 ? 0 : (m == 1 ? m0 : m1));
    if constexpr (ZC) {
      const int c = row / P.nreal, i = row - c * P.nreal;      // row = (case c, row i): h_c is the zero row's
      vec[k] = (m == c) ? P.hz[m][km] : P.hl[m][(int64_t)i * P.hn[m] + km];
    } else {
      vec[k] = P.hl[m][(int64_t)row * P.hn[m] + km];
    }
  }
  if (stB) vec[P.tot + mb] = memr;
  lds_barrier();
  if constexpr (!TAIL) {
    const int q8 = tid & 7;
    for (int o = tid >> 3; o < nout; o += (int)blockDim.x >> 3) {
      const int hd = o / P.zy, c = o - hd * P.zy;
      const float* wr = P.wz[hd] + (int64_t)c * KT;
      float s = 0.0f;
      for (int k = q8; k < KT; k += 8) s = fmaf(wr[k], vec[k], s);
      s = emfn_group_sum(s, 8);
      if (q8 == 0) P.oz[hd][(int64_t)row * P.zy + c] = s + P.bz[hd][c];
    }
  } else {
    // ---- the label tail: zy (the mean head alone) stays in LDS behind the vector; the four small layers ping-pong between two
    // activations [tailw]; y_hat ends in act0
    float* act0 = lds + (KT + 3) / 4 * 4;
    float* act1 = act0 + P.tailw;
    const int fy = P.fy, od = P.od;
    emfn_tail_layer(P.wz[0], P.bz[0], KT, P.zy, vec, act0, false, tid);
    emfn_tail_layer(P.wt[0], P.bt[0], P.zy, fy, act0, act1, true, tid);
    emfn_tail_layer(P.wt[1], P.bt[1], fy, fy, act1, act0, true, tid);
    if constexpr (EMB) {      // fy, the label factor, for the decoders behind this launch (act0 is next written two barriers on)
      for (int o = tid; o < fy; o += blockDim.x) P.emb[(int64_t)row * P.embw + o] = act0[o];
    }
    emfn_tail_layer(P.wt[2], P.bt[2], fy, fy, act0, act1, true, tid);
    emfn_tail_layer(P.wt[3], P.bt[3], fy, od, act1, act0, false, tid);
    for (int o = tid; o < od; o += blockDim.x) P.y_hat[(int64_t)row * od + o] = act0[o];
    if (!P.y || !P.loss || tid >= 64) return;      // (the first wave alone goes on)
    // the row's contribution in a fixed order by one lane; then the arrival ticket of predict_klef_kernel, per chunk: the
    // workgroup that draws the chunk's last ticket adds the chunk's contributions in a fixed order in fp64 -- lane l takes rows
    // l, l + 64, ... ascending, then one fixed butterfly --, carries the running sum of the chunks so far (the launches of a
    // call are stream-ordered), writes the mean behind the last chunk and puts the ticket back to 0.  Nobody waits or spins
    int drawn = 0;
    if (tid == 0) {
      float part = 0.0f;
      if (P.loss_kind == 0) {
        const float* yt = reinterpret_cast<const float*>(P.y) + (int64_t)row * od;
        for (int o = 0; o < od; ++o) part += fabsf(act0[o] - yt[o]);
      } else {
        const int64_t lab = reinterpret_cast<const int64_t*>(P.y)[row];
        float mx = act0[0];
        for (int o = 1; o < od; ++o) mx = fmaxf(mx, act0[o]);
        float se = 0.0f;
        for (int o = 0; o < od; ++o) se += expf(act0[o] - mx);
        const int lc = (int)min(max(lab, (int64_t)0), (int64_t)(od - 1));      // (a label outside [0, od) must not index outside LDS)
        part = (logf(se) + mx) - act0[lc];
      }
      __hip_atomic_store(P.rowloss + row, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      drawn = __hip_atomic_fetch_add(P.ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    }
    drawn = __builtin_amdgcn_readfirstlane(drawn);
    if (drawn != n - 1) return;
    // the last arriver of the chunk: every contribution was stored in front of its workgroup's draw
    double s = 0.0;
    for (int i = tid; i < n; i += 64) s += (double)__hip_atomic_load(P.rowloss + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (tid == 0) {
      if (!P.first) s += __hip_atomic_load(P.acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(P.acc, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (P.last) __hip_atomic_store(P.loss, (float)(s * P.inv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(P.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

struct EmfnSizes { int d[3], z[3], zy, hm[3], M, win, h1, h2, H1, H2, heads; };

static bool emfn_sizes(const int32_t* sz, EmfnSizes& S) {
  if (!sz) return false;
  for (int i = 0; i < 16; ++i)
    if (sz[i] < 1) return false;
  if (sz[16] != 0 && sz[16] != 1) return false;
  for (int i = 0; i < 3; ++i) { S.d[i] = sz[i]; S.z[i] = sz[3 + i]; S.hm[i] = sz[7 + i]; }
  S.zy = sz[6]; S.M = sz[10]; S.win = sz[11]; S.h1 = sz[12]; S.h2 = sz[13]; S.H1 = sz[14]; S.H2 = sz[15]; S.heads = sz[16];
  return true;
}

// the MFN_SIZES sizes of mfm_predict_zeros_mfn, mfm_objective_mfn and mfm_predict_mfn: every one positive (those an entry does not
// use too), heads and the loss kind 0 or 1.  dec: the twelve sizes of mfm_decode_factors
struct MfnSizes { EmfnSizes E; int32_t dec[12]; int fy, od, loss_kind; };

static bool mfn_sizes(const int32_t* sz, MfnSizes& Z) {
  if (!emfn_sizes(sz, Z.E)) return false;
  for (int i = 17; i < 22; ++i)
    if (sz[i] < 1) return false;
  if (sz[22] != 0 && sz[22] != 1) return false;
  const EmfnSizes& S = Z.E;
  const int32_t dec[12] = {S.z[0], S.z[1], S.z[2], S.zy, sz[17], sz[18], sz[19], sz[20], S.d[0], S.d[1], S.d[2], sz[21]};
  memcpy(Z.dec, dec, sizeof(dec));
  Z.fy = sz[20]; Z.od = sz[21]; Z.loss_kind = sz[22];
  return true;
}

static int emfn_pow2_ge(int x) { int p = 1; while (p < x) p <<= 1; return p; }

static size_t emfn_att_lds_floats(const EmfnSizes& S, int CT) {
  const size_t MT = 16 * (size_t)CT, LDP = MT + 4;
  const size_t KCp = round_up(2 * (S.hm[0] + S.hm[1] + S.hm[2]), 16), hbp = round_up(std::max(S.h1, S.h2), 16);
  return (2 * KCp + hbp) * LDP + 2 * EMFN_SPARTS * MT;
}

// ---------------------------------------------------------------- host: the two launches behind the MFN's LSTMs
struct EmfnChain { EmfnAttDev A; EmfnMemDev Mm; int CT, mem_threads; size_t att_lds, mem_lds; };

// what no kernel of an entry covers (MFM_ERR_UNSUPPORTED with the size in the error text): another window, an LSTM beyond the
// resident recurrence.  enc: the entry runs the modality encoders too (z[i] is checked in front of hm[i])
static int mfn_check_covered(const char* who, const EmfnSizes& S, bool enc) {
  if (S.win != 2) {
    set_error("%s: windowsize %d (the attention reads the cell states of exactly 2 steps)", who, S.win);
    return MFM_ERR_UNSUPPORTED;
  }
  for (int i = 0; i < 3; ++i) {
    int rc;
    if (enc && (rc = infer_check_resident(who, S.z[i])) != MFM_OK) return rc;
    if ((rc = infer_check_resident(who, S.hm[i])) != MFM_OK) return rc;
  }
  return MFM_OK;
}

// what the two kernels do not cover (MFM_ERR_UNSUPPORTED with the size in the error text), and their sizing into a zeroed C;
// pairs: the (step, row) pairs of a full chunk's attention chain
// tailw: floats of one activation of the label tail (TAIL; 0: none), two of which lie behind the head's input
static int emfn_chain_check(const char* who, const EmfnSizes& S, int64_t pairs, EmfnChain& C, int tailw = 0) {
  memset(&C, 0, sizeof(C));
  const int tot = S.hm[0] + S.hm[1] + S.hm[2], KC = 2 * tot;
  // the attention chain: 32 pairs per workgroup once 16 would give every CU more than four workgroups, where the LDS allows
  C.CT = ((pairs + 15) / 16 > 4L * device_cus()) ? 2 : 1;
  if (C.CT == 2 && lds_bytes_of(emfn_att_lds_floats(S, 2)) > 160 * 1024) C.CT = 1;
  C.att_lds = lds_bytes_of(emfn_att_lds_floats(S, C.CT));
  if (C.att_lds > 160 * 1024) {
    set_error("%s: %zu bytes of LDS per workgroup of the attention chain (cStar %d wide, hidden layers %d and %d) exceed the 160 KB of a CU",
              who, C.att_lds, KC, S.h1, S.h2);
    return MFM_ERR_UNSUPPORTED;
  }
  // the memory recurrence: its four matrices in registers
  const int QA = emfn_pow2_ge(cdiv(S.M, EMFN_MAXW)), QB = emfn_pow2_ge(cdiv(std::max(S.H1, S.H2), EMFN_MAXW));
  const int nA = (S.H1 + S.H2) * QA, nB = S.M * QB;
  if (QA > 16 || QB > 16 || nA > 1024 || nB > 1024) {
    set_error("%s: memory %d / gamma hidden sizes %d, %d do not fit the register-resident memory recurrence", who, S.M, S.H1, S.H2);
    return MFM_ERR_UNSUPPORTED;
  }
  C.mem_threads = round_up(std::max(nA, nB), 64);
  const int MP = EMFN_MAXW * QA, HP = EMFN_MAXW * QB;
  C.mem_lds = lds_bytes_of(std::max(2 * MP + 2 * HP, round_up(tot + S.M, 4) + 2 * tailw));
  if (C.mem_lds > 160 * 1024) {
    if (tailw)
      set_error("%s: the label head's input of %d + %d floats and two activations of the label tail of %d do not fit the LDS of a CU",
                who, tot, S.M, tailw);
    else
      set_error("%s: the label head's input of %d + %d floats does not fit the LDS of a CU", who, tot, S.M);
    return MFM_ERR_UNSUPPORTED;
  }
  C.Mm.QA = QA; C.Mm.QB = QB; C.Mm.MP = MP; C.Mm.HP = HP;
  return MFM_OK;
}

// sizes and parameters of the two launches: att, the sixteen tensors of the MFN's attention and gamma networks; zyo, those of
// the label head(s), weight and bias each.  The caller sets the records (A.cs / cz, Mm.hl / hz), the chain's buffers (chat, g1p,
// g2p) and Mm.oz
static void emfn_chain_fill_ptrs(EmfnChain& C, const EmfnSizes& S, int T, const float* const* att, const float* const* zyo, int nheads) {
  EmfnAttDev& A = C.A;
  EmfnMemDev& Mm = C.Mm;
  const int tot = S.hm[0] + S.hm[1] + S.hm[2], KC = 2 * tot;
  // att1_fc1, att1_fc2, att2_fc1, att2_fc2, then gamma1_fc1 and gamma2_fc1 (tensors 8 and 12 of the MFN's sixteen)
  static const int att_off[6] = {0, 2, 4, 6, 8, 12};
  for (int l = 0; l < 6; ++l) { A.w[l] = att[att_off[l]]; A.b[l] = att[att_off[l] + 1]; }
  for (int m = 0; m < 3; ++m) { A.hm[m] = S.hm[m]; A.Hpm[m] = round_up(S.hm[m], 16); Mm.hn[m] = S.hm[m]; }
  A.T = T; A.tot = tot; A.KC = KC; A.KCp = round_up(KC, 16); A.h1 = S.h1; A.h2 = S.h2; A.hbp = round_up(std::max(S.h1, S.h2), 16);
  A.M = S.M; A.H1 = S.H1; A.H2 = S.H2;
  Mm.w1m = A.w[4] + KC; Mm.w2m = A.w[5] + KC; Mm.ldw = KC + S.M;
  Mm.w1b = att[10]; Mm.b1b = att[11];
  Mm.w2b = att[14]; Mm.b2b = att[15];
  for (int hd = 0; hd < nheads; ++hd) { Mm.wz[hd] = zyo[2 * hd]; Mm.bz[hd] = zyo[2 * hd + 1]; }
  Mm.T = T; Mm.M = S.M; Mm.H1 = S.H1; Mm.H2 = S.H2; Mm.tot = tot; Mm.zy = S.zy;
  Mm.nheads = nheads;
}
// the same from element offsets into one flat parameter buffer
static void emfn_chain_fill(EmfnChain& C, const EmfnSizes& S, int T, const float* params, const int64_t* att, const int64_t* zyo, int nheads) {
  const float* ap[16];
  const float* zp[4];
  for (int i = 0; i < 16; ++i) ap[i] = params + att[i];
  for (int i = 0; i < 2 * nheads; ++i) zp[i] = params + zyo[i];
  emfn_chain_fill_ptrs(C, S, T, ap, zp, nheads);
}

// the attention chain on a chunk of n rows (ZC: the 3 n rows (case, row)); the memory recurrence reads what it leaves
template <bool ZC>
static int emfn_att_launch(EmfnChain& C, int T, int n, hipStream_t stream) {
  EmfnAttDev& A = C.A;
  EmfnMemDev& Mm = C.Mm;
  const int nv = (ZC ? 3 : 1) * n;
  A.n = n;
  Mm.g1p = A.g1p; Mm.g2p = A.g2p; Mm.chat = A.chat;
  Mm.n = nv; Mm.nreal = n;
  const int64_t np = (int64_t)T * nv;
  if (C.CT == 2)
    return seq_launch_kernel(encode_mfn_att_kernel<2, ZC>, "encode_mfn_att_kernel", dim3((unsigned)((np + 31) / 32)), dim3(EMFN_ATT_THREADS), C.att_lds, stream, nullptr, A);
  return seq_launch_kernel(encode_mfn_att_kernel<1, ZC>, "encode_mfn_att_kernel", dim3((unsigned)((np + 15) / 16)), dim3(EMFN_ATT_THREADS), C.att_lds, stream, nullptr, A);
}

// the memory recurrence on the rows the attention chain was launched on; Mm: C.Mm, or (TAIL) the caller's copy of it with the tail
template <bool ZC, bool TAIL = false, bool EMB = false>
static int emfn_mem_launch(const EmfnChain& C, const std::conditional_t<TAIL, EmfnTailDev, EmfnMemDev>& Mm, hipStream_t stream) {
  if (C.mem_threads <= 512)
    return seq_launch_kernel(encode_mfn_mem_kernel<512, ZC, TAIL, EMB>, "encode_mfn_mem_kernel", dim3(Mm.n), dim3(C.mem_threads), C.mem_lds, stream, nullptr, Mm);
  return seq_launch_kernel(encode_mfn_mem_kernel<1024, ZC, TAIL, EMB>, "encode_mfn_mem_kernel", dim3(Mm.n), dim3(C.mem_threads), C.mem_lds, stream, nullptr, Mm);
}

// the two launches on a chunk of n rows (ZC: the 3 n rows (case, row) behind them)
template <bool ZC>
static int emfn_chain_launch(EmfnChain& C, int T, int n, hipStream_t stream) {
  const int rc = emfn_att_launch<ZC>(C, T, n, stream);
  return rc != MFM_OK ? rc : emfn_mem_launch<ZC>(C, C.Mm, stream);
}

// ---------------------------------------------------------------- host: the MFN's three LSTMs of a call and what lies behind them
// the workspace parts behind the x-projections, in floats and in this order, for chunks of `rows` rows: the c records and last
// hidden states of the MFN's LSTMs, then cHat and the gamma partials of the chain's rows (cases: 1, or the 3 of the zeroed protocol)
struct MfnWs { int64_t cs[3], hl[3], chat, g1p, g2p, total; };
static MfnWs mfn_ws(const EmfnSizes& S, int64_t T, int64_t rows, int cases) {
  MfnWs W;
  W.chat = up4(cases * rows * T * S.M); W.g1p = up4(cases * rows * T * S.H1); W.g2p = up4(cases * rows * T * S.H2);
  W.total = W.chat + W.g1p + W.g2p;
  for (int m = 0; m < 3; ++m) { W.cs[m] = rows * T * hp_of(S.hm[m]); W.hl[m] = up4(rows * S.hm[m]); W.total += W.cs[m] + W.hl[m]; }
  return W;
}

// the first column of modality m in a row of x
static int mfn_col(const EmfnSizes& S, int m) { return m == 0 ? 0 : (m == 1 ? S.d[0] : S.d[0] + S.d[1]); }

// the MFN's lstm l, a, v (MfnLstm: infer_dev.h) of a call, L[0 .. 3) with seq / h_last set by the caller: the cells from their twelve tensors, their
// projections from `gates` on, their c records (A.cs) and last hidden states (Mm.hl) and the chain's buffers from `rest` on in
// the order of mfn_ws; returns the end of those parts
static float* mfn_lstms_fill_ptrs(MfnLstm* L, EmfnChain& C, const EmfnSizes& S, int64_t T, int64_t rows, int cases, const float* const* cells,
                                  float* gates, float* rest) {
  const MfnWs W = mfn_ws(S, T, rows, cases);
  for (int m = 0; m < 3; ++m) {
    const float* const* o = cells + 4 * m;
    seq_fill(*L[m].seq, o[0], o[1], o[2], o[3], S.hm[m], 0);
    L[m].seq->gates = gates; gates += rows * T * 4 * hp_of(S.hm[m]);
    L[m].col = mfn_col(S, m); L[m].d = S.d[m];
  }
  for (int m = 0; m < 3; ++m) { L[m].seq->cs = rest; C.A.cs[m] = rest; rest += W.cs[m]; }
  for (int m = 0; m < 3; ++m) { *L[m].h_last = rest; C.Mm.hl[m] = rest; rest += W.hl[m]; }
  C.A.chat = rest; rest += W.chat;
  C.A.g1p = rest; rest += W.g1p;
  C.A.g2p = rest; rest += W.g2p;
  return rest;
}
// the same from twelve element offsets into one flat parameter buffer
static float* mfn_lstms_fill(MfnLstm* L, EmfnChain& C, const EmfnSizes& S, int64_t T, int64_t rows, int cases, const float* params,
                             const int64_t* cells, float* gates, float* rest) {
  const float* cp[12];
  for (int i = 0; i < 12; ++i) cp[i] = params + cells[i];
  return mfn_lstms_fill_ptrs(L, C, S, T, rows, cases, cp, gates, rest);
}

// ---------------------------------------------------------------- the six recurrences (mfm_encode_mfn; mfm_objective_mfn launches them too)
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

// ---------------------------------------------------------------- host: the six recurrences
static const int kEmfnCanon[EMFN_LSTMS] = {8, 2, 20, 22, 16, 12};      // encoders h = 32 / 8 / 80, the MFN's LSTMs h = 88 / 64 / 48

// the parts of the workspace, in floats, for chunks of `rows` rows: the six x-projections, then mfn_ws
struct EmfnWs { int64_t gates[EMFN_LSTMS], all_gates, total; };
static void emfn_ws(const EmfnSizes& S, int64_t T, int64_t rows, EmfnWs& W) {
  W.all_gates = 0;
  for (int i = 0; i < EMFN_LSTMS; ++i) { W.gates[i] = rows * T * 4 * hp_of(i < 3 ? S.z[i] : S.hm[i - 3]); W.all_gates += W.gates[i]; }
  W.total = W.all_gates + mfn_ws(S, T, rows, 1).total;
}

// the launch(es) of the six recurrences on a chunk of P.n rows: P.d[0 .. EMFN_LSTMS) filled but for block_begin
template <int R>
static int emfn_seq_launch(const char* who, EmfnSeqDev& P, int threads, size_t lds_bytes, hipStream_t stream) {
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

}  // namespace mfm
