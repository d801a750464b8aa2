// The gradient-based interpretation of the factorized model (include/mfm_hip.h, mfm_influence_factors): how strongly the
// factors drive the generation of each modality at each time step,
//   fy[m][t][n] = sum_{i < d_m} sum_{j < fy_size}      (d x_hat_m[t][n][i] / d e[n][j])^2
//   fm[m][t][n] = sum_{i < d_m} sum_{fy_size <= j < h} (d x_hat_m[t][n][i] / d e[n][j])^2,     e = [fy | f_m], h = fy_size + f_m_size,
// of the deterministic eval computation (mfm_model.py:644-656, decoderLSTM :64-91), in FORWARD mode: the h tangent columns of a
// row travel along the decoder's recurrence (gates i, f, g, o; W_s = W_ih + W_hh; h_{-1} = c_{-1} = 0),
//   t = 0:  a = W_ih e + b,        J^a = W_ih              t >= 1:  a = W_s h_{t-1} + b,   J^a = W_s J^h_{t-1}
//   J^c_t = diag(f(1-f) c_{t-1}) J^a_f + diag(f) J^c_{t-1} + diag(i(1-i) g) J^a_i + diag(i(1-g^2)) J^a_g
//   J^h_t = diag(o(1-o) tanh c_t) J^a_o + diag(o(1-tanh^2 c_t)) J^c_t
//   J^x_t = W_fc1 J^h_t,   fy / fm = the sums of squares over its first fy_size / remaining columns.
//
// One small launch per call (influence_pack_kernel) writes the three decoders' weights into the workspace in the order the
// products read them, padded to the MFMA tile with exact zeros: W_ih and W_s as [4 Hp][Hp] with row 4 u + gate (so that one
// 16-row A tile is four units x four gates), b_ih + b_hh alike, W_fc1 as [round_up(d_m, 16)][Hp].  Then, per row chunk, ONE
// launch (influence_kernel) whose workgroups are (decoder m, row tile):
//   * fy and f_m of the tile's rows into LDS on the code path of decode_factors_kernel (stage_rows / dense_rows in the same
//     order): the embedding is bit-identical to the one mfm_decode_factors uses;
//   * the T-step recurrence with h, c, J^h and J^c of the rows in LDS.  J is [unit][row * Hp + column], its rows LDJ = R Hp + 4
//     floats apart (the four k a B fragment reads fall on different banks).  The tangent columns are the N dimension of the
//     products: a tile of R rows shares one stream of W_s and W_fc1 from L2 per step.  A decoder up to Hp = 64 gets R = 4 rows
//     per workgroup, a wider one R = 1 (two 128 x 132 tangents are 135 KB);
//   * J^a = W_s J^h on v_mfma_f32_16x16x4_f32: a wave takes (four units, up to four 16-column tiles); its accumulator holds the
//     four gates of unit u0 + (lane >> 4) for column (lane & 15), so the gate-derivative scalings are lane-local VALU work on
//     coefficients the forward step left in LDS.  J^c is updated in place; J^h_t stays in registers until every wave has read
//     J^h_{t-1}, then it is written (one barrier on either side);
//   * J^x = W_fc1 J^h_t on the same MFMA, 16 outputs x up to four column tiles per task; the squares are added per column in the
//     lane, across the wave's four lane groups by two shuffles, across the waves and then across the columns of a block in LDS,
//     every sum in a fixed order.  Each (block, m, t, row) is stored once, by this workgroup.
// fp32 throughout (exp / tanh from the math library, not the fast forms: the values fall by orders of magnitude over the steps
// and are compared pointwise).  Nothing but the packed weights and the result leaves the chip; no atomics, nothing is handed
// between workgroups: results are bit-identical from run to run, and for any chunking of the rows -- a column's arithmetic
// does not depend on its place in a tile.
#include "infer_dev.h"

namespace mfm {

#define INFL_THREADS 512
#define INFL_WAVES (INFL_THREADS / 64)
#define INFL_CT 4          // 16-column tiles per MFMA task
#define INFL_ITERS 8       // tasks of the recurrent product a wave takes at most (their J^h_t stays in registers)

struct InflOne {
  const float* w[2]; const float* b[2];        // z_m -> f_m: fc1, fc2
  const float* zm;                             // this chunk's rows [n, zs]
  const float* wih_p; const float* ws_p;       // packed [4 Hp][Hp], row 4 u + gate
  const float* bs_p;                           // packed [4 Hp]
  const float* fc_p;                           // packed [Dp][Hp]
  float* out;                                  // (fy block, decoder m, step 0, this chunk's first row) of [2, 3, T, N]
  int zs, fm, h, Hp, R, Dp, block_begin;
};
struct InflDev {
  InflOne d[INFER_DEC];
  const float* wy[2]; const float* by[2];      // zy_to_fy fc1, fc2
  const float* zy;                             // this chunk's rows [n, zys]
  int64_t N, out_block;                        // rows of the whole split; floats from the fy block to the fm block (3 T N)
  int count, T, n, zys, fy, maxw;
};

struct InflPack { const float* w_ih; const float* w_hh; const float* b_ih; const float* b_hh; const float* fcw; float* dst; int h, Hp, d, Dp; };
struct InflPackDev { InflPack p[INFER_DEC]; };

// floats of one decoder's packed weights: W_ih, W_s, b, W_fc1 (each a multiple of 16)
static int64_t infl_pack_floats(int64_t Hp, int64_t Dp) { return 8 * Hp * Hp + 4 * Hp + Dp * Hp; }

__global__ __launch_bounds__(256) void influence_pack_kernel(const InflPackDev P) {
  const InflPack& p = P.p[blockIdx.y];
  const int h = p.h, Hp = p.Hp;
  const int nW = 4 * Hp * Hp, total = 2 * nW + 4 * Hp + p.Dp * Hp;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    float v = 0.0f;
    if (e < 2 * nW) {
      const int f = e < nW ? e : e - nW;
      const int row = f / Hp, k = f - row * Hp, u = row >> 2, g = row & 3;
      if (u < h && k < h) {
        const int64_t o = ((int64_t)g * h + u) * h + k;
        v = p.w_ih[o];
        if (e >= nW) v += p.w_hh[o];
      }
    } else if (e < 2 * nW + 4 * Hp) {
      const int row = e - 2 * nW, u = row >> 2, g = row & 3;
      if (u < h) v = p.b_ih[g * h + u] + p.b_hh[g * h + u];
    } else {
      const int f = e - 2 * nW - 4 * Hp;
      const int row = f / Hp, k = f - row * Hp;
      if (row < p.d && k < h) v = p.fcw[(int64_t)row * h + k];
    }
    p.dst[e] = v;
  }
}

// acc[ct] += A[16 x K] . J[K x 16 columns of tile ct], K = 16 kchunks.  a: this lane's row of the packed A, at k = 4 (lane >> 4);
// b: J at row 4 (lane >> 4), the lane's column of the first tile.  MFMA step s of chunk c multiplies k = 16 c + 4 (lane >> 4) + s
// on both sides: the four steps' A values arrive as one 16-byte load, the next chunk's while this one multiplies
__device__ __forceinline__ void infl_product(const float* __restrict__ a, const float* b, const int LDJ, const int kchunks, const int nct,
                                             f32x4 (&acc)[INFL_CT]) {
  f32x4 a4 = *reinterpret_cast<const f32x4*>(a);
  for (int c = 0; c < kchunks; ++c) {
    const f32x4 an = *reinterpret_cast<const f32x4*>(a + 16 * (c + 1 < kchunks ? c + 1 : c));
    const float* bc = b + (int64_t)16 * c * LDJ;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int ct = 0; ct < INFL_CT; ++ct)
        if (ct < nct) acc[ct] = mma16x16x4(a4[s], bc[s * LDJ + 16 * ct], acc[ct]);
    }
    a4 = an;
  }
}

__device__ __forceinline__ float infl_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int R>
__device__ __forceinline__ void influence_body(const InflDev& P, const InflOne& D, const int tile, float* lds) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, q = lane >> 4;
  const int h = D.h, Hp = D.Hp, fy = P.fy, b0 = tile * R;
  const int NC = R * Hp, LDJ = NC + 4, NT = NC / 16, HR = Hp * R;
  float* Jh = lds;                             // [Hp][LDJ]
  float* Jc = Jh + Hp * LDJ;
  float* coef = Jc + Hp * LDJ;                 // [6][Hp][R]: on J^a_i, J^a_f, J^a_g, J^a_o, J^c_{t-1}, J^c_t
  float* hv = coef + 6 * HR;                   // [Hp][R]: the embedding [fy | f_m], then h_t
  float* cv = hv + HR;                         // [Hp][R]
  float* av = cv + HR;                         // [4 Hp][R], row 4 u + gate
  float* red = av + 4 * HR;                    // [waves][NC]
  float* csum = red + INFL_WAVES * NC;         // [NC]
  float* zin = csum + NC;                      // [maxw][R]
  float* t0 = zin + P.maxw * R;                // [maxw][R]

  // the embedding, as decode_factors_kernel computes it
  stage_rows<R>(P.zy, P.zys, b0, P.n, zin);
  dense_rows<R>(P.wy[0], P.by[0], P.zys, fy, zin, t0, true);
  dense_rows<R>(P.wy[1], P.by[1], fy, fy, t0, hv, true);
  stage_rows<R>(D.zm, D.zs, b0, P.n, zin);
  dense_rows<R>(D.w[0], D.b[0], D.zs, D.fm, zin, t0, true);
  dense_rows<R>(D.w[1], D.b[1], D.fm, D.fm, t0, hv + fy * R, true);
  for (int e = h * R + tid; e < HR; e += INFL_THREADS) hv[e] = 0.0f;      // pad units
  for (int e = tid; e < HR; e += INFL_THREADS) cv[e] = 0.0f;
  lds_barrier();

  const int kchunks = Hp / 16, UG = Hp / 4, nctg = (NT + INFL_CT - 1) / INFL_CT, ntask = UG * nctg, DT = D.Dp / 16;
  for (int t = 0; t < P.T; ++t) {
    // ---- the forward step: a, the gates, c_t, h_t, and the six scalings of the tangents
    dense_rows<R>(t == 0 ? D.wih_p : D.ws_p, D.bs_p, Hp, 4 * Hp, hv, av, false);
    for (int e = tid; e < HR; e += INFL_THREADS) {
      const int u = e / R, r = e - u * R;
      const float* ar = av + 4 * u * R + r;
      const float i = infl_sigmoid(ar[0]), f = infl_sigmoid(ar[R]), g = tanhf(ar[2 * R]), o = infl_sigmoid(ar[3 * R]);
      const float cp = cv[e];
      const float c = f * cp + i * g;
      const float tc = tanhf(c);
      cv[e] = c;
      hv[e] = o * tc;
      coef[e] = i * (1.0f - i) * g;
      coef[HR + e] = f * (1.0f - f) * cp;
      coef[2 * HR + e] = i * (1.0f - g * g);
      coef[3 * HR + e] = o * (1.0f - o) * tc;
      coef[4 * HR + e] = f;
      coef[5 * HR + e] = o * (1.0f - tc * tc);
    }
    lds_barrier();

    // ---- J^a = W_s J^h_{t-1} (step 0: W_ih itself), J^c_t in place, J^h_t in registers
    // (the task loop stays rolled -- unrolled, its eight bodies spill -- and hn is indexed by comparing the uniform `it`)
    float hn[INFL_ITERS][INFL_CT];
#pragma unroll
    for (int k = 0; k < INFL_ITERS; ++k)
#pragma unroll
      for (int ct = 0; ct < INFL_CT; ++ct) hn[k][ct] = 0.0f;
#pragma unroll 1
    for (int it = 0; it < INFL_ITERS; ++it) {
      const int task = wave + it * INFL_WAVES;
      if (task < ntask) {
        // (column group first: the groups of a decoder differ in size, and this way every wave gets its share of each)
        const int cg = task / UG, u0 = 4 * (task - cg * UG), ct0 = cg * INFL_CT, nct = min(INFL_CT, NT - ct0);
        f32x4 acc[INFL_CT];
#pragma unroll
        for (int ct = 0; ct < INFL_CT; ++ct) acc[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (t == 0) {
#pragma unroll
          for (int ct = 0; ct < INFL_CT; ++ct)
            if (ct < nct) {
              const int n = 16 * (ct0 + ct) + col, j = n % Hp;
              const float* wr = D.wih_p + (int64_t)4 * (u0 + q) * Hp + j;
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[ct][r] = wr[r * Hp];
            }
        } else {
          infl_product(D.ws_p + (int64_t)(4 * u0 + col) * Hp + 4 * q, Jh + 4 * q * LDJ + 16 * ct0 + col, LDJ, kchunks, nct, acc);
        }
        const int u = u0 + q;
        float v[INFL_CT];
#pragma unroll
        for (int ct = 0; ct < INFL_CT; ++ct) {
          v[ct] = 0.0f;
          if (ct < nct) {
            const int n = 16 * (ct0 + ct) + col;
            const int e = u * R + (R == 1 ? 0 : n / Hp);
            const float jc_old = t > 0 ? Jc[u * LDJ + n] : 0.0f;
            const float jc = coef[e] * acc[ct][0] + coef[HR + e] * acc[ct][1] + coef[2 * HR + e] * acc[ct][2] + coef[4 * HR + e] * jc_old;
            Jc[u * LDJ + n] = jc;
            v[ct] = coef[3 * HR + e] * acc[ct][3] + coef[5 * HR + e] * jc;
          }
        }
#pragma unroll
        for (int k = 0; k < INFL_ITERS; ++k)
          if (it == k) {
#pragma unroll
            for (int ct = 0; ct < INFL_CT; ++ct) hn[k][ct] = v[ct];
          }
      }
    }
    lds_barrier();
#pragma unroll 1
    for (int it = 0; it < INFL_ITERS; ++it) {
      const int task = wave + it * INFL_WAVES;
      if (task < ntask) {
        const int cg = task / UG, u0 = 4 * (task - cg * UG), ct0 = cg * INFL_CT, nct = min(INFL_CT, NT - ct0);
        float v[INFL_CT];
#pragma unroll
        for (int ct = 0; ct < INFL_CT; ++ct) v[ct] = 0.0f;
#pragma unroll
        for (int k = 0; k < INFL_ITERS; ++k)
          if (it == k) {
#pragma unroll
            for (int ct = 0; ct < INFL_CT; ++ct) v[ct] = hn[k][ct];
          }
#pragma unroll
        for (int ct = 0; ct < INFL_CT; ++ct)
          if (ct < nct) Jh[(u0 + q) * LDJ + 16 * (ct0 + ct) + col] = v[ct];
      }
    }
    lds_barrier();

    // ---- J^x = W_fc1 J^h_t, squared and added per column
    for (int cg = 0; cg < nctg; ++cg) {
      const int ct0 = cg * INFL_CT, nct = min(INFL_CT, NT - ct0);
      float sq[INFL_CT];
#pragma unroll
      for (int ct = 0; ct < INFL_CT; ++ct) sq[ct] = 0.0f;
      for (int dt = wave; dt < DT; dt += INFL_WAVES) {
        f32x4 acc[INFL_CT];
#pragma unroll
        for (int ct = 0; ct < INFL_CT; ++ct) acc[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        infl_product(D.fc_p + (int64_t)(16 * dt + col) * Hp + 4 * q, Jh + 4 * q * LDJ + 16 * ct0 + col, LDJ, kchunks, nct, acc);
#pragma unroll
        for (int ct = 0; ct < INFL_CT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) sq[ct] = fmaf(acc[ct][r], acc[ct][r], sq[ct]);
      }
#pragma unroll
      for (int ct = 0; ct < INFL_CT; ++ct)
        if (ct < nct) {
          float v = sq[ct];
          v += __shfl_xor(v, 16);
          v += __shfl_xor(v, 32);
          if (q == 0) red[wave * NC + 16 * (ct0 + ct) + col] = v;
        }
    }
    lds_barrier();
    for (int n = tid; n < NC; n += INFL_THREADS) {
      float v = red[n];
#pragma unroll
      for (int w = 1; w < INFL_WAVES; ++w) v += red[w * NC + n];
      csum[n] = v;
    }
    lds_barrier();
    // ---- the columns of a block: one wave per (row, block), lanes over the columns, then a butterfly
    for (int p = wave; p < 2 * R; p += INFL_WAVES) {
      const int r = p >> 1, blk = p & 1;
      const int j1 = blk ? h : fy;
      float v = 0.0f;
      for (int j = (blk ? fy : 0) + lane; j < j1; j += 64) v += csum[r * Hp + j];
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
      if (lane == 0 && b0 + r < P.n) D.out[blk * P.out_block + (int64_t)t * P.N + b0 + r] = v;
    }
    // (csum and red are next written behind the barriers of the next step's forward part)
  }
}

__global__ __launch_bounds__(INFL_THREADS) void influence_kernel(const InflDev P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int bid = blockIdx.x;
  MFM_SEQ_BLOCK_LSTM(P, bid, di)
  const InflOne& D = P.d[di];
  if (D.R == 4) influence_body<4>(P, D, bid - D.block_begin, lds);
  else influence_body<1>(P, D, bid - D.block_begin, lds);
}

// ---------------------------------------------------------------- host
// rows per workgroup of a decoder with padded hidden size Hp: what keeps the two tangents in LDS and a wave's share of the
// recurrent product within INFL_ITERS tasks
static int infl_tile_rows(int Hp) { return Hp <= 64 ? 4 : 1; }

static size_t infl_lds_floats(int Hp, int R, int maxw) {
  const size_t NC = (size_t)R * Hp;
  return 2 * (size_t)Hp * (NC + 4) + 12 * NC + (INFL_WAVES + 1) * NC + 2 * (size_t)maxw * R;
}

static int64_t infl_ws_floats(const int32_t* sz) {
  int64_t t = 0;
  for (int m = 0; m < INFER_DEC; ++m) t += infl_pack_floats(hp_of(sz[7] + sz[4 + m]), hp_of(sz[8 + m]));
  return t;
}

static int influence_factors(int T, int64_t N, const int32_t* sz, const float* params, const int64_t* offs, const float* const* z,
                             float* ws, float* out, int64_t max_rows, hipStream_t stream) {
  static const char* who = "influence factors";
  MFM_REQUIRE(sz && params && offs && z && ws && out, "%s: bad arguments (sizes, params, offsets, factors, workspace and output must not be null)", who);
  int rc = infer_check_sizes(who, T, N, sz);
  if (rc != MFM_OK) return rc;
  for (int i = 0; i < 4; ++i) MFM_REQUIRE(z[i] && ((uintptr_t)z[i] & 3) == 0, "%s: factor %d is null or not 4-byte aligned", who, i);
  MFM_REQUIRE((((uintptr_t)params | (uintptr_t)ws) & 15) == 0 && ((uintptr_t)out & 3) == 0,
              "%s: params and workspace must be 16-byte aligned, the output 4-byte aligned", who);
  if ((rc = infer_check_rows(who, N, max_rows)) != MFM_OK) return rc;
  if ((rc = infer_check_offsets(who, offs, 38, 6, 16, 34)) != MFM_OK) return rc;
  const int zys = sz[3], fy = sz[7];
  const int rows = (int)gen_rows(N, max_rows);
  int maxw = std::max(zys, fy);
  for (int m = 0; m < INFER_DEC; ++m) {
    if ((rc = infer_check_resident(who, fy + sz[4 + m])) != MFM_OK) return rc;
    maxw = std::max(maxw, std::max(fy + sz[4 + m], sz[m]));
  }
  InflDev P;
  InflPackDev K;
  memset(&P, 0, sizeof(P));
  memset(&K, 0, sizeof(K));
  size_t lds_bytes = 0;
  int64_t pack_max = 0;
  float* w0 = ws;
  for (int m = 0; m < INFER_DEC; ++m) {
    InflOne& D = P.d[m];
    const int64_t* o = offs + 16 + 6 * m;
    D.h = fy + sz[4 + m]; D.Hp = round_up(D.h, 16); D.Dp = round_up(sz[8 + m], 16); D.R = infl_tile_rows(D.Hp);
    D.zs = sz[m]; D.fm = sz[4 + m];
    const size_t lb = lds_bytes_of(infl_lds_floats(D.Hp, D.R, maxw));
    if ((rc = infer_check_lds(who, lb, maxw, D.R, D.h)) != MFM_OK) return rc;
    lds_bytes = std::max(lds_bytes, lb);
    const int ntask = (D.Hp / 4) * cdiv(D.R * D.Hp / 16, INFL_CT);
    MFM_REQUIRE(ntask <= INFL_ITERS * INFL_WAVES, "%s: internal: %d product tasks for h = %d", who, ntask, D.h);
    for (int l = 0; l < 2; ++l) { D.w[l] = params + offs[4 + 4 * m + 2 * l]; D.b[l] = params + offs[5 + 4 * m + 2 * l]; }
    const int64_t nW = 4 * (int64_t)D.Hp * D.Hp;
    D.wih_p = w0; D.ws_p = w0 + nW; D.bs_p = w0 + 2 * nW; D.fc_p = w0 + 2 * nW + 4 * D.Hp;
    K.p[m] = InflPack{params + o[0], params + o[1], params + o[2], params + o[3], params + o[4], w0, D.h, D.Hp, sz[8 + m], D.Dp};
    const int64_t pf = infl_pack_floats(D.Hp, D.Dp);
    pack_max = std::max(pack_max, pf);
    w0 += pf;
  }
  for (int l = 0; l < 2; ++l) { P.wy[l] = params + offs[2 * l]; P.by[l] = params + offs[2 * l + 1]; }
  P.count = INFER_DEC; P.T = T; P.zys = zys; P.fy = fy; P.maxw = maxw;
  P.N = N; P.out_block = (int64_t)INFER_DEC * T * N;

  hipLaunchKernelGGL(influence_pack_kernel, dim3((unsigned)std::min<int64_t>((pack_max + 255) / 256, 256), INFER_DEC), dim3(256), 0, stream, K);
  MFM_LAUNCH_CHECK("influence_pack_kernel");
  for (int64_t n0 = 0; n0 < N; n0 += rows) {
    const int n = (int)std::min<int64_t>(rows, N - n0);
    int blocks = 0;
    for (int m = 0; m < INFER_DEC; ++m) {
      InflOne& D = P.d[m];
      D.zm = z[m] + n0 * sz[m];
      D.out = out + (int64_t)m * T * N + n0;
      D.block_begin = blocks;
      blocks += cdiv(n, D.R);
    }
    P.zy = z[3] + n0 * zys;
    P.n = n;
    if ((rc = seq_launch_kernel(influence_kernel, "influence_kernel", dim3(blocks), dim3(INFL_THREADS), lds_bytes, stream, nullptr, P)) != MFM_OK)
      return rc;
  }
  return MFM_OK;
}

}  // namespace mfm

extern "C" int64_t mfm_influence_factors_workspace_floats(int32_t T, int64_t N, const int32_t* sizes, int64_t max_rows) {
  if (T < 1 || N < 1 || !sizes || max_rows < 0) return 0;
  for (int i = 0; i < 12; ++i)
    if (sizes[i] < 1) return 0;
  return mfm::infl_ws_floats(sizes);
}

extern "C" int mfm_influence_factors(int32_t T, int64_t N, const int32_t* sizes, const float* params, const int64_t* offsets,
                                     const float* const* z, float* workspace, float* out, int64_t max_rows, void* stream) {
  return mfm::influence_factors(T, N, sizes, params, offsets, z, workspace, out, max_rows, (hipStream_t)stream);
}
