// Prediction of the ablations M_B and M_D (include/mfm_hip.h, mfm_predict_ablation): what the `evaluate` / `predict` blocks of the
// reference's train_mfm_ablation report -- y_hat, its label loss and (M_B) the three reconstruction errors -- on what those
// numbers depend on alone.  Both classes run three independent own-modality encoders that meet at the label head:
//   family 0, M_B   z_m = encoder_m(x_m), f_m = relu(fc2(relu(fc1(z_m)))); y_hat = fy_to_y_fc2(relu(fy_to_y_fc1([f_l | f_a | f_v])));
//                   gen_m = mse(decoder_m(f_m, T), x_m)
//   family 1, M_D   the same encoders and z -> f MLPs; y_hat = fs_to_y([f_l | f_a | f_v]); no decoders
// Per row chunk, on one stream:
//   1. the three input projections on their column ranges of x as ONE grouped GEMM (mfn_xproj_chunk, infer_dev.h);
//   2. ablation_encode_kernel, ONE launch: workgroup (encoder m, row tile) runs the T-step recurrence, the encoder's fc1 and the
//      z -> f MLP with everything in LDS, stores its f_m rows into the chunk's [n, fl + fa + fv] block and draws the tile's
//      arrival ticket.  The workgroup that draws the LAST of a tile's three tickets reads the tile's rows of the block back,
//      runs the label head, writes the tile's rows of y_hat and, with labels, one loss contribution per row, and puts the ticket
//      word back to 0.  z_m never leaves the chip.  The last tile of the chunk to finish (a second ticket, per chunk) adds the
//      chunk's contributions in a fixed order in fp64 onto the running sum and, behind the last chunk, writes the mean;
//   3. with gen: ablation_decode_kernel (ablation_dec_dev.h), workgroup (decoder m, row tile) stages its f_m rows and runs the decoder form of the
//      recurrence with h = f_m, storing h_t alone; fc1_sqerr_kernel (objective.hip) over the stored h against x, one partial per
//      workgroup; zeros_finish_kernel (zeros.hip) adds the partials in fp64 in a fixed order.
// Nobody waits or spins: a workgroup draws its ticket and either leaves or goes on, so the launch does not depend on which
// workgroups are resident together.  No float atomics touch a result: y_hat, disc and gen are bit-identical from run to run for a
// given (T, N, max_rows); a row's arithmetic does not depend on its place in a tile or a chunk, nor on which workgroup drew the
// last ticket, so y_hat is bit-identical for every chunking within one tile-row form.  Launches 2 and 3 follow the launch rules
// of infer_dev.h: the per-block switch for the canonical size tuple only, else one launch per LSTM -- the tickets then meet across
// the three launches, which are stream-ordered.
#include "ablation_dec_dev.h"

namespace mfm {

#define ABL_FAMILIES 2
#define ABL_MOD_PTRS 16      // per modality: 6 of encoder_m, 4 of z<m>_to_f<m>, 6 of decoder_m
#define ABL_NPARAM (ABL_MODS * ABL_MOD_PTRS + 4)

struct AblOne {
  SeqDev seq;                                  // gates (the x-projections, read only), w_hh, h = z_m, Hp, hk4
  const float* w[3]; const float* b[3];        // the encoder's fc1, z<m>_to_f<m> fc1, fc2
  int fm, col, block_begin;                    // f_m, and its first column in a row of the f block
};
struct AblEncDev {
  AblOne d[ABL_MODS];
  const float* wy[2]; const float* by[2];      // the label head: fy_to_y fc1, fc2 (M_B); fs_to_y, null (M_D)
  float* f;                                    // workspace: this chunk's [n, ftot] rows of [f_l | f_a | f_v]
  float* y_hat; const void* y;                 // this chunk's rows [n, od] and labels (null: no loss)
  float* rowloss; double* acc;                 // workspace: one contribution per row of the chunk, the running sum
  int* tile_ticket; int* chunk_ticket;         // workspace: one arrival word per row tile, one per chunk
  float* disc;
  double inv;                                  // 1 / (N od) (L1) or 1 / N (CE): the WHOLE split
  int count, T, n, maxw, ftot, fy, od, headw, flag_off, loss_kind, first, last;
};

template <int R, int K0, int K1, int K2>
__global__ __launch_bounds__(1024) void ablation_encode_kernel(const AblEncDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, bid = blockIdx.x;
  MFM_SEQ_BLOCK_LSTM(P, bid, di)
  const AblOne& E = P.d[di];
  const int tile = bid - E.block_begin, b0 = tile * R;
  const float* hT = nullptr;
  MFM_TUPLE3(hT = small_fwd_body<KQ, R, false, false, false>(E.seq, P.T, P.n, tile, lds))
  // the two h buffers stay where they are; two activations behind them ([maxw][R] each): z_m and f_m in the first, the MLP's
  // hidden layer in the second
  float* act0 = lds + 2 * E.seq.Hp * R;
  float* act1 = act0 + P.maxw * R;
  const int h = E.seq.h, fm = E.fm, ftot = P.ftot, n = P.n;
  dense_rows<R>(E.w[0], E.b[0], h, h, hT, act0, false);
  dense_rows<R>(E.w[1], E.b[1], h, fm, act0, act1, true);
  dense_rows<R>(E.w[2], E.b[2], fm, fm, act1, act0, true);
  for (int e = tid; e < fm * R; e += blockDim.x) {
    const int r = e / fm, o = e - r * fm;
    if (b0 + r < n) __hip_atomic_store(P.f + (int64_t)(b0 + r) * ftot + E.col + o, act0[o * R + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // the tile's arrival ticket (the pattern of predict_klef_kernel): every wave's stores above have been acknowledged in front
  // of the barrier (a barrier alone does not wait for global stores: common.h), the draw's release comes behind it; the XCDs
  // do not share an L2, hence agent scope on the stores, the draw and the loads below
  int* flag = reinterpret_cast<int*>(lds + P.flag_off);      // (4 floats behind everything else this kernel lays out)
  sync_stores();
  if (tid == 0) flag[0] = __hip_atomic_fetch_add(P.tile_ticket + tile, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (flag[0] != ABL_MODS - 1) return;
  // ---- the last of the tile's three arrivers: the other two modalities' rows were stored in front of their draws
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  float* fin = lds;                            // [ftot][R], over the recurrence's buffers, which nobody reads any more
  float* h0 = fin + ftot * R;                  // [headw][R] each
  float* h1 = h0 + P.headw * R;
  for (int e = tid; e < ftot * R; e += blockDim.x) {
    const int r = e / ftot, k = e - r * ftot;
    fin[k * R + r] = (b0 + r < n) ? __hip_atomic_load(P.f + (int64_t)(b0 + r) * ftot + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0f;
  }
  lds_barrier();
  const int od = P.od;
  if (P.wy[1]) {
    dense_rows<R>(P.wy[0], P.by[0], ftot, P.fy, fin, h0, true);
    dense_rows<R>(P.wy[1], P.by[1], P.fy, od, h0, h1, false);
  } else {
    dense_rows<R>(P.wy[0], P.by[0], ftot, od, fin, h1, false);
  }
  store_rows<R>(h1, P.y_hat, od, b0, n, tid);
  if (!P.y) {
    if (tid == 0) __hip_atomic_store(P.tile_ticket + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  // a row's contribution in a fixed order by one lane; then the chunk's ticket as encode_mfn_mem_kernel<.., TAIL> draws it, per
  // tile: the last tile of the chunk adds the chunk's contributions in a fixed order in fp64 -- lane l takes rows l, l + 64, ...
  // ascending, then one fixed butterfly --, carries the running sum of the chunks so far (the launches of a call are
  // stream-ordered), writes the mean behind the last chunk and puts the ticket back to 0
  if (tid < R && b0 + tid < n) {
    const int row = b0 + tid;
    float part = 0.0f;
    if (P.loss_kind == 0) {
      const float* yt = reinterpret_cast<const float*>(P.y) + (int64_t)row * od;
      for (int o = 0; o < od; ++o) part += fabsf(h1[o * R + tid] - yt[o]);
    } else {
      const int64_t lab = reinterpret_cast<const int64_t*>(P.y)[row];
      float mx = h1[tid];
      for (int o = 1; o < od; ++o) mx = fmaxf(mx, h1[o * R + tid]);
      float se = 0.0f;
      for (int o = 0; o < od; ++o) se += expf(h1[o * R + tid] - mx);
      const int lc = (int)min(max(lab, (int64_t)0), (int64_t)(od - 1));      // (a label outside [0, od) must not index outside LDS)
      part = (logf(se) + mx) - h1[lc * R + tid];
    }
    __hip_atomic_store(P.rowloss + row, part, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  sync_stores();
  if (tid == 0) {
    __hip_atomic_store(P.tile_ticket + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    flag[0] = __hip_atomic_fetch_add(P.chunk_ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (flag[0] != (n + R - 1) / R - 1 || tid >= 64) return;      // (the first wave of the chunk's last tile alone goes on)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double s = 0.0;
  for (int i = tid; i < n; i += 64) s += (double)__hip_atomic_load(P.rowloss + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  if (tid == 0) {
    if (!P.first) s += __hip_atomic_load(P.acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(P.acc, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (P.last) __hip_atomic_store(P.disc, (float)(s * P.inv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(P.chunk_ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// the ticket words of a call start at 0: a launch, so that a captured graph orders it like every other node of the call
__global__ __launch_bounds__(256) void ablation_zero_kernel(int* words, const int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) words[i] = 0;
}

// ---------------------------------------------------------------- host
static const int kAblEnc[ABL_MODS] = {8, 2, 20};          // the canonical sizes: the encoders h = zl / za / zv = 32 / 8 / 80 (the decoders'
                                                          // h = fl / fa / fv = 88 / 8 / 8: hk4 22 / 2 / 2 where their launch is named)

template <int R>
static int abl_encode_launch(const char* who, AblEncDev& P, int threads, size_t lds_bytes, hipStream_t stream) {
  bool canon = true;
  for (int i = 0; i < ABL_MODS; ++i) canon = canon && P.d[i].seq.hk4 == kAblEnc[i];
  return infer_launch_tuple_or_each<R>(who, "ablation_encode_kernel", P, canon ? ablation_encode_kernel<R, 8, 2, 20> : nullptr,
                                       [](auto kk) { return ablation_encode_kernel<R, decltype(kk)::value, 0, 0>; }, threads, lds_bytes, stream);
}

struct AblSizes { int z[ABL_MODS], fm[ABL_MODS], dm[ABL_MODS], fy, od, D, ftot; };
// false: a size below 1
static bool abl_sizes(const int32_t* sz, AblSizes& S) {
  if (!sz) return false;
  for (int i = 0; i < 12; ++i)
    if (sz[i] < 1) return false;
  for (int m = 0; m < ABL_MODS; ++m) { S.z[m] = sz[m]; S.fm[m] = sz[4 + m]; S.dm[m] = sz[8 + m]; }
  S.fy = sz[7]; S.od = sz[11];
  S.D = S.dm[0] + S.dm[1] + S.dm[2];
  S.ftot = S.fm[0] + S.fm[1] + S.fm[2];
  return true;
}

// the workspace, in this order (every part a multiple of 4 floats; include/mfm_hip.h states it term by term): the chunk's three
// x-projections; its f block; with gen the decoders' stored h, the squared-error partials and the ZER_ACC fp64 accumulators;
// with labels one loss contribution per chunk row; one ticket word per chunk row; the fp64 running sum, the chunk's ticket and a pad
struct AblLayout { int64_t f, hs, part, acc, row, ticket, tail, total; };
static AblLayout abl_layout(int64_t T, int64_t N, const AblSizes& S, bool with_gen, bool with_labels, int64_t max_rows) {
  const int64_t rows = gen_rows(N, max_rows);
  AblLayout o;
  o.f = 0;
  for (int m = 0; m < ABL_MODS; ++m) o.f += rows * T * 4 * hp_of(S.z[m]);
  o.hs = o.f + up4(rows * S.ftot);
  o.part = o.hs;
  for (int m = 0; with_gen && m < ABL_MODS; ++m) o.part += rows * T * hp_of(S.fm[m]);
  o.acc = o.part + (with_gen ? up4(fc1_sqerr_tiles(T, rows, S.dm)) : 0);
  o.row = o.acc + (with_gen ? up4(2 * ZER_ACC) : 0);
  o.ticket = o.row + (with_labels ? up4(rows) : 0);
  o.tail = o.ticket + up4(rows);
  o.total = o.tail + 4;
  return o;
}

// rows per workgroup of the encoders' launch and of the decoders' (0: none)
static void abl_tile_rows(bool with_gen, int rows, int* Re, int* Rd) {
  *Re = gen_tile_rows(ABL_MODS, rows);
  *Rd = with_gen ? gen_tile_rows(ABL_MODS, rows) : 0;
}

static int predict_ablation(int T, int64_t N, const int32_t* sz, int family, int loss_kind, int with_gen, const float* const* prm,
                            const float* x, const void* y, float* ws, float* y_hat, float* gen, float* disc, int64_t max_rows,
                            hipStream_t stream) {
  static const char* who = "predict ablation";
  MFM_REQUIRE(sz && prm && x && ws && y_hat, "%s: bad arguments (sizes, parameter table, x, workspace and y_hat must not be null)", who);
  MFM_REQUIRE(family >= 0 && family < ABL_FAMILIES, "%s: family = %d (0 M_B, 1 M_D)", who, family);
  int rc = infer_check_sizes(who, T, N, sz);
  if (rc != MFM_OK) return rc;
  if ((rc = infer_check_loss_kind(who, loss_kind)) != MFM_OK) return rc;
  if ((rc = infer_check_rows(who, N, max_rows)) != MFM_OK) return rc;
  MFM_REQUIRE(with_gen == 0 || with_gen == 1, "%s: with_gen = %d (0 or 1)", who, with_gen);
  MFM_REQUIRE(family == 0 || (!with_gen && !gen), "%s: family 1 (M_D) has no decoders: with_gen must be 0 and gen null", who);
  MFM_REQUIRE((with_gen != 0) == (gen != nullptr), "%s: with_gen and gen come together (both, or neither)", who);
  MFM_REQUIRE((y != nullptr) == (disc != nullptr), "%s: labels and disc come together (both, or both null)", who);
  // (x is read 16 bytes at a time by the grouped GEMM alone, which takes dword-aligned addresses, and element by element as the
  // squared error's target; the recurrences read the workspace 16 bytes at a time)
  MFM_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)ws & 15) == 0, "%s: x must be 4-byte aligned, the workspace 16-byte aligned", who);
  MFM_REQUIRE((((uintptr_t)y_hat | (uintptr_t)gen | (uintptr_t)disc) & 3) == 0 && ((uintptr_t)y & (loss_kind == 0 ? 3 : 7)) == 0,
              "%s: y_hat, gen, disc or the labels are misaligned", who);
  AblSizes S;
  abl_sizes(sz, S);
  for (int m = 0; m < ABL_MODS; ++m)
    for (int i = 0; i < (with_gen ? ABL_MOD_PTRS : 10); ++i) {
      const float* p = prm[m * ABL_MOD_PTRS + i];
      MFM_REQUIRE(p, "%s: parameter %d of modality %d is null", who, i, m);
      const bool lstm_w = i == 0 || i == 1 || i == 10 || i == 11;
      MFM_REQUIRE(((uintptr_t)p & (lstm_w ? 15 : 3)) == 0, "%s: parameter %d of modality %d is misaligned (LSTM weights 16 bytes, the rest 4)", who, i, m);
    }
  const float* const* head = prm + ABL_MODS * ABL_MOD_PTRS;
  for (int i = 0; i < (family == 0 ? 4 : 2); ++i)
    MFM_REQUIRE(head[i] && ((uintptr_t)head[i] & 3) == 0, "%s: label-head parameter %d is null or misaligned", who, i);

  const int rows = (int)gen_rows(N, max_rows);
  int Re, Rd;
  abl_tile_rows(with_gen != 0, rows, &Re, &Rd);
  int enc_maxw = 1, enc_threads = 64, dec_threads = 64, maxhp = 16, maxf = 1;
  size_t dec_seq = 0;
  for (int m = 0; m < ABL_MODS; ++m) {
    if ((rc = infer_check_resident(who, S.z[m])) != MFM_OK) return rc;
    if (with_gen && (rc = infer_check_resident(who, S.fm[m])) != MFM_OK) return rc;
    enc_maxw = std::max(enc_maxw, std::max(S.z[m], S.fm[m]));
    enc_threads = std::max(enc_threads, 8 * round_up(S.z[m], 16));
    maxhp = std::max(maxhp, round_up(S.z[m], 16));
    if (with_gen) {
      dec_threads = std::max(dec_threads, 8 * round_up(S.fm[m], 16));
      dec_seq = std::max(dec_seq, seq_lds_floats(S.fm[m], Rd));
      maxhp = std::max(maxhp, round_up(S.fm[m], 16));
      maxf = std::max(maxf, S.fm[m]);
    }
  }
  // the layout rule of the LDS: an encoder workgroup keeps the two h buffers and puts two activations [maxw][R] behind them; the
  // tile's last arriver lays the row of f and the head's two activations over all of that; the ticket's answer behind both
  const int headw = family == 0 ? std::max(S.fy, S.od) : S.od;
  size_t enc_floats = 0;
  for (int m = 0; m < ABL_MODS; ++m) enc_floats = std::max(enc_floats, enc_lds_floats(S.z[m], Re, 2, enc_maxw));
  const size_t head_floats = ((size_t)S.ftot + 2 * (size_t)headw) * Re;
  const size_t flag_off = (std::max(enc_floats, head_floats) + 3) / 4 * 4;
  const size_t enc_lds = lds_bytes_of(flag_off + 4);
  if (head_floats > enc_floats && enc_lds > 160 * 1024) {
    set_error("%s: the label head's input row of fl + fa + fv = %d floats and its activations (widest %d, %d rows per workgroup) exceed the 160 KB of LDS of a CU",
              who, S.ftot, headw, Re);
    return MFM_ERR_UNSUPPORTED;
  }
  const size_t dec_lds = with_gen ? lds_bytes_of(dec_seq + (size_t)maxf * Rd) : 0;
  if ((rc = infer_check_lds(who, std::max(enc_lds, dec_lds), enc_lds > dec_lds ? enc_maxw : maxf, enc_lds > dec_lds ? Re : Rd)) != MFM_OK) return rc;
  if ((rc = infer_check_chunk(who, rows, T, std::max(S.D, 4 * maxhp), "projection")) != MFM_OK) return rc;
  MFM_REQUIRE((int64_t)rows * S.ftot < ((int64_t)1 << 31), "%s: a chunk of %d rows is too large; pass a row cap", who, rows);
  MFM_REQUIRE(!with_gen || fc1_sqerr_tiles(T, rows, S.dm) < ((int64_t)1 << 31), "%s: a chunk of %d rows x %d steps is too large; pass a row cap", who, rows, T);

  // ---- everything that does not depend on the chunk
  const AblLayout lay = abl_layout(T, N, S, with_gen != 0, y != nullptr, max_rows);
  AblEncDev PE;
  AblDecDev PD;
  Fc1SqLaunch Sq;
  memset(&PE, 0, sizeof(PE));
  memset(&PD, 0, sizeof(PD));
  memset(&Sq, 0, sizeof(Sq));
  MfnLstm L[ABL_MODS];
  float* gates = ws;
  float* hs = ws + lay.hs;
  Sq.hmax = 1;
  for (int m = 0, col = 0, fcol = 0; m < ABL_MODS; ++m) {
    const float* const* p = prm + m * ABL_MOD_PTRS;
    AblOne& E = PE.d[m];
    seq_fill(E.seq, p[0], p[1], p[2], p[3], S.z[m], 0);
    E.seq.gates = gates; gates += (int64_t)rows * T * 4 * E.seq.Hp;
    E.w[0] = p[4]; E.b[0] = p[5];
    for (int l = 0; l < 2; ++l) { E.w[1 + l] = p[6 + 2 * l]; E.b[1 + l] = p[7 + 2 * l]; }
    E.fm = S.fm[m]; E.col = fcol;
    L[m] = MfnLstm{&E.seq, nullptr, col, S.dm[m]};
    if (with_gen) {
      AblDec& Dd = PD.d[m];
      seq_fill(Dd.seq, p[10], p[11], p[12], p[13], S.fm[m], 1);
      Dd.seq.hs = hs; hs += (int64_t)rows * T * Dd.seq.Hp;
      Dd.col = fcol;
      Fc1SqItem& I = Sq.F.it[m];
      I.hs = Dd.seq.hs; I.w = p[14]; I.bias = p[15];
      I.d = S.dm[m]; I.h = Dd.seq.h; I.Hp = Dd.seq.Hp; I.col_tiles = cdiv(S.dm[m], OBJ_BN);
      Sq.hmax = std::max(Sq.hmax, Dd.seq.h);
    }
    Sq.col[m] = col;
    Sq.inv_gen[m] = 1.0 / ((double)T * (double)N * (double)S.dm[m]);
    col += S.dm[m]; fcol += S.fm[m];
  }
  Sq.F.D = S.D; Sq.F.N = N; Sq.T = T;
  PE.wy[0] = head[0]; PE.by[0] = head[1];
  if (family == 0) { PE.wy[1] = head[2]; PE.by[1] = head[3]; }
  PE.f = ws + lay.f;
  PE.rowloss = ws + lay.row;
  PE.tile_ticket = reinterpret_cast<int*>(ws + lay.ticket);
  PE.acc = reinterpret_cast<double*>(ws + lay.tail);      // (a multiple of 4 floats from a 16-byte aligned base)
  PE.chunk_ticket = reinterpret_cast<int*>(ws + lay.tail + 2);
  PE.disc = disc;
  PE.inv = inv_label_count(loss_kind, N, S.od);
  PE.count = ABL_MODS; PE.T = T; PE.maxw = enc_maxw; PE.ftot = S.ftot; PE.fy = S.fy; PE.od = S.od; PE.headw = headw;
  PE.flag_off = (int)flag_off; PE.loss_kind = loss_kind;
  PD.f = PE.f; PD.count = ABL_MODS; PD.T = T; PD.ftot = S.ftot; PD.seq_floats = (int)dec_seq;

  ZerFinishDev Q;
  memset(&Q, 0, sizeof(Q));
  for (int m = 0; m < ABL_MODS; ++m) Q.inv_gen[m] = Sq.inv_gen[m];
  Q.acc = reinterpret_cast<double*>(ws + lay.acc);
  Q.gen = gen;
  Q.od = S.od; Q.loss_kind = loss_kind;      // (no labels here: the label loss is the tickets')
  float* part = ws + lay.part;
  // the ticket words start at 0 (the workspace's contents are arbitrary, and a call that ended in an error between two launches
  // may have left arrivals behind); every last arriver puts its word back
  const int nwords = (int)(lay.total - lay.ticket);
  if ((rc = seq_launch_kernel(ablation_zero_kernel, "ablation_zero_kernel", dim3(cdiv(nwords, 256)), dim3(256), 0, stream, nullptr,
                              reinterpret_cast<int*>(ws + lay.ticket), nwords)) != MFM_OK)
    return rc;

  for (int64_t n0 = 0; n0 < N; n0 += rows) {
    const int n = (int)std::min<int64_t>(rows, N - n0);
    if ((rc = mfn_xproj_chunk(ABL_MODS, L, x, T, N, S.D, n0, n, stream)) != MFM_OK) return rc;
    PE.n = n;
    PE.y_hat = y_hat + n0 * S.od;
    PE.y = labels_at(y, loss_kind, n0, S.od);
    PE.first = n0 == 0; PE.last = n0 + n == N;
    rc = (Re == 1) ? abl_encode_launch<1>(who, PE, enc_threads, enc_lds, stream) : abl_encode_launch<4>(who, PE, enc_threads, enc_lds, stream);
    if (rc != MFM_OK) return rc;
    if (!with_gen) continue;
    PD.n = n;
    rc = (Rd == 1) ? abl_decode_launch<1, 22, 2, 2>(who, PD, dec_threads, dec_lds, stream) : abl_decode_launch<4, 22, 2, 2>(who, PD, dec_threads, dec_lds, stream);
    if (rc != MFM_OK) return rc;
    if ((rc = fc1_sqerr_chunk(Sq, x, n0, n, part, Q.part, Q.npart, stream)) != MFM_OK) return rc;
    Q.n = n; Q.first = n0 == 0; Q.last = n0 + n == N;
    if ((rc = zeros_finish_launch(Q, stream)) != MFM_OK) return rc;
  }
  return MFM_OK;
}

}  // namespace mfm

extern "C" int64_t mfm_predict_ablation_workspace_floats(int32_t T, int64_t N, const int32_t* sizes, int32_t family, int32_t with_gen,
                                                         int32_t with_labels, int64_t max_rows) {
  mfm::AblSizes S;
  if (T < 1 || N < 1 || family < 0 || family >= ABL_FAMILIES || max_rows < 0 || with_gen < 0 || with_gen > 1 || (family == 1 && with_gen) ||
      !mfm::abl_sizes(sizes, S))
    return 0;
  return mfm::abl_layout(T, N, S, with_gen != 0, with_labels != 0, max_rows).total;
}

extern "C" int mfm_predict_ablation_tile_rows(int64_t N, int32_t family, int32_t with_gen, int64_t max_rows, int32_t* tile_rows) {
  if (N < 1 || max_rows < 0 || !tile_rows || family < 0 || family >= ABL_FAMILIES || with_gen < 0 || with_gen > 1 || (family == 1 && with_gen)) {
    mfm::set_error("predict ablation tile rows: bad arguments (N %lld, family %d, with_gen %d, row cap %lld)", (long long)N, family, with_gen,
                   (long long)max_rows);
    return MFM_ERR_ARG;
  }
  const int rows = (int)std::min<int64_t>(mfm::gen_rows(N, max_rows), INT32_MAX);
  int Re, Rd;
  mfm::abl_tile_rows(with_gen != 0, rows, &Re, &Rd);
  tile_rows[0] = Re; tile_rows[1] = Rd;
  return MFM_OK;
}

extern "C" int mfm_predict_ablation(int32_t T, int64_t N, const int32_t* sizes, int32_t family, int32_t loss_kind, int32_t with_gen,
                                    const float* const* params, const float* x, const void* y, float* workspace, float* y_hat,
                                    float* gen, float* disc, int64_t max_rows, void* stream) {
  return mfm::predict_ablation(T, N, sizes, family, loss_kind, with_gen, params, x, y, workspace, y_hat, gen, disc, max_rows,
                               (hipStream_t)stream);
}
