// The full validation objective of MFM_KL and MFM (include/mfm_hip.h, mfm_objective_mfn): what mfm_objective_klef (objective.hip)
// is for MFM_KL_EF, for the classes whose label factor comes from the Memory Fusion Network (mfm_model.py:140-199, :723-743),
//     loss = disc + lda_xl mse_l + lda_xa mse_a + lda_xv mse_v + lda_mmd reg
// from the deterministic eval forward -- no plan, no training workspace, no x_hat.  reg is the sum of the four loss_KLD(mu,
// logvar) with heads ("kl"), and without ("mmd") the sum over the four factors of the maximum mean discrepancy against a
// Gaussian sample the caller passes (mfm_model.py:14-34): mean K(g, g) + mean K(z, z) - 2 mean K(g, z), K(a, b) =
// exp(-|a - b|^2 / dim^2), over all N^2 pairs of the WHOLE split.  Per row chunk of n rows, on one stream:
//   1. the encoder half exactly as mfm_encode_mfn launches it (encode_mfn_front.h): the grouped projection GEMM, the six
//      recurrences in one launch, the attention chain, the memory recurrence with the label head(s).  With heads the chunk's
//      means and log-variances go to the workspace; without, the means go to their rows [n0, n0 + n) of four whole-split
//      arrays [N, size] in the workspace, because the MMD needs every row;
//   2. decode_factors_kernel on the chunk's means: the three decoders' h_t (in the place of the projections, which are dead by
//      then) and y_hat of the chunk into the workspace;
//   3. fc1_sqerr_kernel against the real x (objective.hip);
//   4. objective_finish_kernel (objective.hip): the chunk's squared-error partials, label-loss sum and, with heads, KLD sum in
//      fp64 in a fixed order into the accumulators; with heads it writes the six floats behind the last chunk;
//   5. without heads, once behind the last chunk: objective_mfn_mmd_kernel -- workgroup (term, tile of MI rows i) stages its
//      rows of z and g, walks j in tiles of 32 rows staged in LDS (odd row stride), forms the three kernel values of a pair and
//      adds kzz + kgg - 2 kgz per pair (the cancellation happens in the small numbers), lane -> wave (DPP) -> workgroup (LDS) in
//      a fixed order, ONE partial into its own slot -- and objective_mfn_mmd_finish_kernel, which adds the partials of each term
//      in ascending order in fp64, scales by 1 / N^2, forms the total and writes the six floats.
// No gradient, no [N, N] scratch, no float atomics: the six results are bit-identical from run to run for a given (T, N,
// max_rows) and, without heads, a given gauss.  The parser of the MFN_SIZES sizes (mfn_sizes) is that of encode_mfn_dev.h.
#include "encode_mfn_front.h"

namespace mfm {

#define OMFN_JT 32          // rows j per LDS tile of the MMD

struct OmfnMmdTerm { const float* z; const float* g; int dim, pad_; };      // z [N, dim] contiguous; g: rows ldg apart
struct OmfnMmdDev { OmfnMmdTerm t[4]; float* partials; int64_t ldg; int N; };

// MI rows i per workgroup; the 256 threads are MI rows x NS = 256 / MI slices of the j tile, PJ columns each.  MI = 32 is the
// throughput shape; MI = 8 serves small splits (N = 32: 16 workgroups instead of 4)
template <int MI>
__global__ __launch_bounds__(256) void objective_mfn_mmd_kernel(const OmfnMmdDev P) {
  constexpr int NS = 256 / MI, PJ = OMFN_JT / NS;
  static_assert(PJ >= 1 && NS * PJ == OMFN_JT, "slices must tile the j tile");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float red[4];
  const OmfnMmdTerm& M = P.t[blockIdx.y];
  const float* __restrict__ z = M.z;
  const float* __restrict__ g = M.g;
  const int dim = M.dim, N = P.N;
  const int ld = dim | 1;                         // odd row stride: conflict-free when lanes walk rows
  float* zi = lds;                                // [MI][ld]
  float* gi = zi + MI * ld;
  float* zj = gi + MI * ld;                       // [OMFN_JT][ld]
  float* gj = zj + OMFN_JT * ld;
  const int tid = threadIdx.x;
  const int il = tid & (MI - 1), js = tid / MI;
  const int i0 = blockIdx.x * MI;
  const float inv_k2 = 1.0f / ((float)dim * (float)dim);

  for (int e = tid; e < MI * dim; e += 256) {
    const int r = e / dim, c = e - r * dim;
    const int64_t row = min(i0 + r, N - 1);       // (rows past the edge: a copy of the last one, masked below)
    zi[r * ld + c] = z[row * dim + c];
    gi[r * ld + c] = g[row * P.ldg + c];
  }
  const bool ilive = i0 + il < N;
  const float* zr = zi + il * ld;
  const float* gr = gi + il * ld;
  float part = 0.0f;
  for (int j0 = 0; j0 < N; j0 += OMFN_JT) {
    __syncthreads();                              // the previous tile is consumed (and zi / gi are visible)
    for (int e = tid; e < OMFN_JT * dim; e += 256) {
      const int r = e / dim, c = e - r * dim;
      const int64_t row = min(j0 + r, N - 1);
      zj[r * ld + c] = z[row * dim + c];
      gj[r * ld + c] = g[row * P.ldg + c];
    }
    __syncthreads();
    float dzz[PJ], dgz[PJ], dgg[PJ];
#pragma unroll
    for (int jj = 0; jj < PJ; ++jj) dzz[jj] = dgz[jj] = dgg[jj] = 0.0f;
    for (int c = 0; c < dim; ++c) {
      const float a = zr[c], p = gr[c];
#pragma unroll
      for (int jj = 0; jj < PJ; ++jj) {
        const float b = zj[(js * PJ + jj) * ld + c], q = gj[(js * PJ + jj) * ld + c];
        dzz[jj] = fmaf(a - b, a - b, dzz[jj]);
        dgz[jj] = fmaf(a - q, a - q, dgz[jj]);
        dgg[jj] = fmaf(p - q, p - q, dgg[jj]);
      }
    }
#pragma unroll
    for (int jj = 0; jj < PJ; ++jj)
      if (ilive && j0 + js * PJ + jj < N)
        part += (expf(-dzz[jj] * inv_k2) + expf(-dgg[jj] * inv_k2)) - 2.0f * expf(-dgz[jj] * inv_k2);
  }
  part = wave_sum_dpp(part);
  if ((tid & 63) == 0) red[tid >> 6] = part;
  __syncthreads();
  if (tid == 0) P.partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

struct OmfnMmdFinishDev {
  const float* partials; int per_term;           // [4][per_term]
  const double* acc;                             // the OBJ_ACC sums of objective_finish_kernel over the whole split
  float* out;
  double inv_gen[INFER_DEC], inv_disc, inv_n2;
  float lda[4];
};

__global__ __launch_bounds__(64) void objective_mfn_mmd_finish_kernel(const OmfnMmdFinishDev P) {
  __shared__ double term[4];
  const int tid = threadIdx.x;
  if (tid < 4) {
    const float* p = P.partials + (int64_t)tid * P.per_term;
    double s = 0.0;
    for (int i = 0; i < P.per_term; ++i) s += (double)p[i];
    term[tid] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  const float reg = (float)((((term[0] + term[1]) + term[2]) + term[3]) * P.inv_n2);
  const float d = (float)(P.acc[4] * P.inv_disc);
  const float gl = (float)(P.acc[0] * P.inv_gen[0]), ga = (float)(P.acc[1] * P.inv_gen[1]), gv = (float)(P.acc[2] * P.inv_gen[2]);
  P.out[0] = d + P.lda[0] * gl + P.lda[1] * ga + P.lda[2] * gv + P.lda[3] * reg;
  P.out[1] = d; P.out[2] = gl; P.out[3] = ga; P.out[4] = gv; P.out[5] = reg;
}

// ---------------------------------------------------------------- host
// rows i per workgroup of the MMD, and its workgroups (= partial slots) per term
static int omfn_mmd_rows(int64_t N) { return N <= 256 ? 8 : 32; }
static int64_t omfn_mmd_tiles(int64_t N) { return (N + omfn_mmd_rows(N) - 1) / omfn_mmd_rows(N); }

// the workspace, in this order (every part a multiple of 4 floats; include/mfm_hip.h states it term by term): the chunk's six
// x-projections and, behind the recurrences, the decoders' h in the same place; the parts of mfm_encode_mfn behind its
// projections (c records, last hidden states, cHat, the gamma partials); the factors -- with heads the chunk's four means and
// four log-variances, without the four whole-split means; the chunk's y_hat; its squared-error partials; without heads the
// MMD's partials; the fp64 accumulators
struct OmfnLayout { int64_t o_cs, zpart[4], o_z, o_yhat, o_part, o_mmd, o_acc, total; };
static OmfnLayout omfn_layout(const MfnSizes& Z, int64_t T, int64_t N, int64_t max_rows) {
  const EmfnSizes& S = Z.E;
  const int64_t rows = gen_rows(N, max_rows);
  OmfnLayout L;
  EmfnWs W;
  emfn_ws(S, T, rows, W);
  L.o_cs = std::max(W.all_gates, decode_ws_floats(T, N, Z.dec[7], Z.dec[4], Z.dec[5], Z.dec[6], max_rows));
  L.o_z = L.o_cs + (W.total - W.all_gates);
  int64_t zf = 0;
  for (int i = 0; i < 4; ++i) { L.zpart[i] = up4((S.heads ? rows : N) * Z.dec[i]); zf += L.zpart[i]; }
  L.o_yhat = L.o_z + (S.heads ? 2 : 1) * zf;
  L.o_part = L.o_yhat + up4(rows * Z.dec[11]);
  L.o_mmd = L.o_part + up4(fc1_sqerr_tiles(T, rows, Z.dec + 8));
  L.o_acc = L.o_mmd + (S.heads ? 0 : up4(4 * omfn_mmd_tiles(N)));
  L.total = L.o_acc + up4(2 * OBJ_ACC);
  return L;
}

static int objective_mfn(int T, int64_t N, const int32_t* sz, const float* lambdas, const float* params, const int64_t* offs,
                         const float* x, const void* y, const float* gauss, float* ws, float* out, int64_t max_rows, hipStream_t stream) {
  static const char* who = "objective mfn";
  MfnSizes Z;
  MFM_REQUIRE(T >= 1 && N >= 1 && mfn_sizes(sz, Z),
              "%s: sizes must be positive (T %d, N %lld, and the %d sizes; heads and the loss kind 0 or 1)", who, T, (long long)N, MFN_SIZES);
  MFM_REQUIRE(lambdas && params && offs && x && y && ws && out,
              "%s: bad arguments (lambdas, params, offsets, x, y, workspace and out must not be null)", who);
  const EmfnSizes& S = Z.E;
  MFM_REQUIRE(S.heads || gauss, "%s: bad arguments (without heads the Gaussian sample must not be null)", who);
  MFM_REQUIRE(!S.heads || !gauss, "%s: bad arguments (with heads there is no MMD: the Gaussian sample must be null)", who);
  MFM_REQUIRE(((uintptr_t)gauss & 3) == 0, "%s: gauss must be 4-byte aligned", who);
  int rc = infer_check_aligned(who, params, x, ws);
  if (rc != MFM_OK) return rc;
  // (the row cap, the offsets of mfm_encode_mfn and its refusals: emfn_front_prepare; the 38 offsets of mfm_decode_factors
  // behind them: decode_factors_prepare)
  const OmfnLayout lay = omfn_layout(Z, T, N, max_rows);
  EmfnFront F;
  if ((rc = emfn_front_prepare(who, T, N, S, params, offs, ws, ws + lay.o_cs, max_rows, F)) != MFM_OK) return rc;
  const int od = Z.od, loss_kind = Z.loss_kind, rows = F.rows, o_dec = F.n_offs;
  DecLaunch Dl;
  Fc1SqLaunch Sq;
  if ((rc = decode_factors_prepare(who, T, N, Z.dec, params, offs + o_dec, ws, max_rows, Dl)) != MFM_OK) return rc;
  if ((rc = fc1_sqerr_prepare(who, Dl, N, Sq)) != MFM_OK) return rc;
  const int MI = omfn_mmd_rows(N);
  size_t mmd_lds = 0;
  if (!S.heads) {
    int dmax = 1;
    for (int i = 0; i < 4; ++i) dmax = std::max(dmax, (int)Z.dec[i]);
    mmd_lds = lds_bytes_of((size_t)(2 * MI + 2 * OMFN_JT) * (dmax | 1));
    if (mmd_lds > 160 * 1024) {
      set_error("%s: %zu bytes of LDS per workgroup of the MMD (widest factor %d) exceed the 160 KB of a CU", who, mmd_lds, dmax);
      return MFM_ERR_UNSUPPORTED;
    }
  }

  // ---- everything that does not depend on the chunk
  // heads: zbuf[0 .. 4) the chunk's means, [4 .. 8) its log-variances; no heads: zbuf[0 .. 4) the whole split's means
  float* zbuf[8] = {nullptr};
  {
    float* p = ws + lay.o_z;
    for (int half = 0; half < (S.heads ? 2 : 1); ++half)
      for (int i = 0; i < 4; ++i) { zbuf[4 * half + i] = p; p += lay.zpart[i]; }
  }
  float* y_hat = ws + lay.o_yhat;
  float* part = ws + lay.o_part;
  double* acc = reinterpret_cast<double*>(ws + lay.o_acc);      // (a multiple of 4 floats from a 16-byte aligned base)

  ObjFinishDev Q;
  memset(&Q, 0, sizeof(Q));
  for (int m = 0; m < INFER_DEC; ++m) Q.inv_gen[m] = Sq.inv_gen[m];
  Q.y_hat = y_hat; Q.acc = acc; Q.out = out;
  Q.inv_disc = inv_label_count(loss_kind, N, od);
  for (int i = 0; i < 4; ++i) Q.lda[i] = lambdas[i];
  Q.od = od; Q.loss_kind = loss_kind;

  for (int64_t n0 = 0; n0 < N; n0 += rows) {
    const int n = (int)std::min<int64_t>(rows, N - n0);
    // this chunk's first rows of the four means (and log-variances)
    float* zc[8];
    for (int i = 0; i < 8; ++i) zc[i] = (zbuf[i] && !S.heads) ? zbuf[i] + n0 * Z.dec[i & 3] : zbuf[i];
    if ((rc = emfn_front_chunk(who, F, x, N, n0, n, zc, stream)) != MFM_OK) return rc;
    // (the projections are dead behind the recurrences: the decoders' h takes their place)
    if ((rc = decode_factors_chunk(who, Dl, zc, y_hat, n, stream)) != MFM_OK) return rc;
    if ((rc = fc1_sqerr_chunk(Sq, x, n0, n, part, Q.part, Q.npart, stream)) != MFM_OK) return rc;
    for (int i = 0; i < 4; ++i) { Q.mu[i] = zc[i]; Q.lv[i] = zc[4 + i]; Q.nz[i] = S.heads ? n * Z.dec[i] : 0; }
    Q.y = labels_at(y, loss_kind, n0, od);
    Q.n = n; Q.first = n0 == 0; Q.last = S.heads && n0 + n == N;      // (without heads the MMD's finish writes the results)
    if ((rc = objective_finish_launch(Q, stream)) != MFM_OK) return rc;
  }
  if (S.heads) return MFM_OK;

  // ---- the MMD over the whole split
  OmfnMmdDev G;
  memset(&G, 0, sizeof(G));
  int gcol = 0;
  for (int i = 0; i < 4; ++i) {
    G.t[i].z = zbuf[i]; G.t[i].g = gauss + gcol; G.t[i].dim = Z.dec[i];
    gcol += Z.dec[i];
  }
  G.ldg = gcol; G.N = (int)N;
  G.partials = ws + lay.o_mmd;
  const int tiles = (int)omfn_mmd_tiles(N);
  if (MI == 8)
    rc = seq_launch_kernel(objective_mfn_mmd_kernel<8>, "objective_mfn_mmd_kernel", dim3(tiles, 4), dim3(256), mmd_lds, stream, nullptr, G);
  else
    rc = seq_launch_kernel(objective_mfn_mmd_kernel<32>, "objective_mfn_mmd_kernel", dim3(tiles, 4), dim3(256), mmd_lds, stream, nullptr, G);
  if (rc != MFM_OK) return rc;
  OmfnMmdFinishDev Fin;
  memset(&Fin, 0, sizeof(Fin));
  Fin.partials = G.partials; Fin.per_term = tiles; Fin.acc = acc; Fin.out = out;
  for (int m = 0; m < INFER_DEC; ++m) Fin.inv_gen[m] = Sq.inv_gen[m];
  Fin.inv_disc = Q.inv_disc;
  Fin.inv_n2 = 1.0 / ((double)N * (double)N);
  for (int i = 0; i < 4; ++i) Fin.lda[i] = lambdas[i];
  return seq_launch_kernel(objective_mfn_mmd_finish_kernel, "objective_mfn_mmd_finish_kernel", dim3(1), dim3(64), 0, stream, nullptr, Fin);
}

}  // namespace mfm

extern "C" int64_t mfm_objective_mfn_workspace_floats(int32_t T, int64_t N, const int32_t* sizes, int64_t max_rows) {
  mfm::MfnSizes Z;
  if (T < 1 || N < 1 || max_rows < 0 || !sizes || !mfm::mfn_sizes(sizes, Z)) return 0;
  return mfm::omfn_layout(Z, T, N, max_rows).total;
}

extern "C" int mfm_objective_mfn_tile_rows(int64_t N, int64_t max_rows) {
  if (N < 1 || max_rows < 0) return -1;
  return mfm::gen_tile_rows(EMFN_LSTMS, (int)mfm::gen_rows(N, max_rows));
}

extern "C" int mfm_objective_mfn(int32_t T, int64_t N, const int32_t* sizes, const float* lambdas, const float* params,
                                 const int64_t* offsets, const float* x, const void* y, const float* gauss, float* workspace,
                                 float* out, int64_t max_rows, void* stream) {
  return mfm::objective_mfn(T, N, sizes, lambdas, params, offsets, x, y, gauss, workspace, out, max_rows, (hipStream_t)stream);
}
