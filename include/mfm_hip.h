/*
 * mfm_hip.h -- C ABI of libmfm_hip.so: the MI355X (gfx950 / CDNA4) implementation of the
 * MFM training hot path of pliang279/factorized.
 *
 * The reference has no FFI / plugin boundary: it is pure Python and all arithmetic lives in
 * PyTorch ops (nn.LSTMCell, nn.Linear, autograd, optim.Adam).  The drop-in boundary is
 * therefore the Python class surface (factorized_amd/mfm_model.py mirrors mfm_model.py); THIS
 * header is the native boundary underneath it -- what a maintainer of the reference would bind
 * with ctypes.  Each entry point names the reference code it replaces
 * (file:line into the reference repo).
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; every pointer is a DEVICE pointer unless it says host.
 *   - caller owns every buffer (PyTorch caching allocator); nothing here allocates device memory
 *     that outlives a call.  Workspace sizes come from mfm_plan_workspace_bytes().
 *   - all work is enqueued on the hipStream_t passed as `stream` (void*, 0 = default stream) and
 *     the call returns immediately; no hidden synchronisation (the reference only syncs at
 *     `.item()`, mfm_mosi.py:442).
 *   - return 0 on success, negative MFM_ERR_* otherwise; mfm_last_error() gives the text.
 *     No C++ exception crosses this boundary.
 *   - fp32 everywhere; LSTM gate order is torch's i,f,g,o; weight layouts are torch's
 *     (weight_ih [4h,d], weight_hh [4h,h], Linear.weight [out,in]), row-major.
 *   - "padded hidden" Hp = round_up(h,16).  Sequence state buffers use the padded layouts
 *       gates [T,B,4,Hp]   hs [T,B,Hp]   cs [T,B,Hp]
 *     pad units hold exact zeros for h/c (0.5/0/0.5 gates); pad rows do not exist (B is exact).
 */
#ifndef MFM_HIP_H_
#define MFM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFM_OK 0
#define MFM_ERR_ARG (-1)
#define MFM_ERR_HIP (-2)
#define MFM_ERR_UNSUPPORTED (-3)

#define MFM_ABI_VERSION 5

int mfm_abi_version(void);
const char* mfm_last_error(void);
/* number of CUs of the current device (for grid heuristics / reporting). */
int mfm_device_cus(void);

/* ------------------------------------------------------------------------------------------
 * Grouped fp32 GEMM on the f32 MFMA (v_mfma_f32_16x16x4_f32), exact fp32 FMA chains.
 *   for z in [0,batch):  C[z][m][n] (+)= alpha * sum_k A(z,m,k) * B(z,k,n) + bias[z][n] + bias2[z][n]
 * A(z,m,k) = a[z*a_sz + m*a_sm + k*a_sk], B(z,k,n) = b[z*b_sz + k*b_sk + n*b_sn],
 * C element at c[z*c_sz + m*ldc + n].  Columns n in [n_valid, n) (pad units) are produced as exact zeros
 * by a plain product and are left untouched when accumulate!=0; columns [n, ldc) are never written.
 * accumulate!=0 -> atomic += into c (and c2 if non-null), needed for split_k>1.  The biases are added once
 * whatever the split, and alpha scales the product only, not the biases.  k = 0 is a valid problem
 * (C = bias, or C += bias): a and b must still be non-null and address at least one element.
 * Operands: strides are >= 0, and the span of one batch member of a or b, first to last element, is at most
 * 2^31 - 1 BYTES (2^29 - 1 fp32 elements): the tile loads carry 32-bit byte offsets; a larger span is refused
 * (MFM_ERR_ARG) with the operand and its span in the message.  fp32 base pointers need 4-byte alignment only.
 * What the loads touch: an operand that is unit-stride along k (or along m for a, n for b) is fetched 16 bytes
 * at a time, so up to three elements BEHIND a row's K range, or behind m / n_valid of an m-/n-contiguous
 * operand, are read when they lie inside the operand's span (the columns of a wider matrix an operand is a
 * slice of, the next row), and are then multiplied by zero.  Those elements must be FINITE: an inf or NaN
 * there survives the multiply and poisons the output row / column.  Where they may not be finite (missing
 * values next to observed ones), gather the operand into a zero-padded matrix of its own first, as
 * csrc/impute.hip does.  Nothing is read outside the span.
 * Replaces every nn.Linear / LSTMCell addmm and its AddmmBackward on the path:
 * mfm_model.py:56,83,85 (x W_ih^T hoisted over all T), :61,90 (fc1), autograd of the same.
 */
typedef struct MfmGemmDesc {
  const float* a; const float* b; float* c; float* c2;
  const float* bias; const float* bias2;
  int64_t a_sz, a_sm, a_sk;
  int64_t b_sz, b_sk, b_sn;
  int64_t c_sz, ldc, bias_sz;
  int32_t m, n, k, n_valid, batch, split_k, accumulate;
  float alpha;
  /* bf16-RESIDENT operands (ABI 2; mfm_gemm_grouped_bf16 only, 0 = the fp32 buffers described above).  A bf16 plan keeps
   * its saved activations in HBM as bf16 (plan.hip): a_bf16 -> `a` points to __bf16 elements (strides count bf16
   * elements; the unit-stride axis must start on 16-byte boundaries), loaded straight into the LDS image without a
   * rounding pass; c_bf16 -> `c` (and c2) receive bf16 (nearest even) instead of fp32 -- plain, non-accumulating
   * products only. */
  int32_t a_bf16, c_bf16;
  int32_t reserved_[2];   /* MUST be zero (memset the struct first): used inside the library; the entry points reject anything else */
} MfmGemmDesc;

int mfm_gemm_grouped_f32(const MfmGemmDesc* descs /*host*/, int count, void* stream);
/* The same products with bf16 MFMA operands (v_mfma_f32_16x16x32_bf16) and fp32 accumulation: a and b are still
 * fp32 buffers, rounded to bf16 (nearest even) on the way from the global tile to LDS; c, bias, alpha, the
 * epilogue and the atomics are fp32 exactly as above.  "bf16 compute, fp32 master weights" of BASELINE.json
 * configs 2-4.  A group holding an operand that is not unit-stride along m/n or k runs on the fp32 kernel -- every
 * problem of that launch (at most MFM_GEMM_MAXP consecutive descriptors), with fp32 results -- and is refused if it
 * also holds an a_bf16 / c_bf16 descriptor. */
int mfm_gemm_grouped_bf16(const MfmGemmDesc* descs /*host*/, int count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Whole-sequence LSTM recurrence (one persistent workgroup per 16 batch rows per LSTM; weights
 * stay in VGPRs for all T steps, h is exchanged through LDS, c never leaves registers).
 * Up to MFM_MAX_SEQ independent LSTMs run in ONE launch.
 *
 * Encoder form (is_dec=0), replaces encoderLSTM.forward's time loop mfm_model.py:47-58:
 *   in : gates = x_t W_ih^T + b_ih + b_hh for all t (from mfm_gemm_grouped_f32), w_hh
 *   out: gates <- activated (i,f,g,o), hs, cs.
 * Decoder form (is_dec=1), replaces decoderLSTM.forward's loop mfm_model.py:72-88:
 *   step 0 consumes h_init [B, ld_init] through w_ih from zero state; steps >=1 feed the
 *   hidden state back as the input, i.e. gates = h (W_ih+W_hh)^T + b_ih + b_hh.
 */
#define MFM_MAX_SEQ 6
typedef struct MfmSeqDesc {
  float* gates; float* hs; float* cs;
  const float* w_hh; const float* w_ih; const float* b_ih; const float* b_hh;
  const float* h_init; int64_t ld_init;
  /* backward only */
  const float* dh_ext;   /* dec: [T,B,Hp] grad wrt every h_t; enc: [B, ld_dh] grad wrt h_{T-1} */
  int64_t ld_dh;
  float* d_h_init;       /* dec: [B, ld_dinit] out (grad wrt h_init); enc: unused */
  int64_t ld_dinit;
  int32_t h, is_dec;
  const float* dc_ext;   /* optional [T,B,Hp]: external grad wrt every CELL state c_t (the MFN encoder
                            reads c_t, mfm_model.py:171-173); NULL for the plain encoders/decoders */
  void* w_pack;          /* bf16 entry points only, optional: mfm_lstm_pack_bytes(h, is_dec) bytes filled by
                            mfm_lstm_pack_bf16 from the CURRENT weights (bf16 MFMA fragments in lane order); NULL =
                            the recurrence kernels gather their fragments from the fp32 matrices themselves (slow) */
  /* ABI 2, bf16 entry points only: bf16-RESIDENT saved activations.  store_bf16 != 0 -> `gates` (x-projection in,
     activated gates / dA out), `hs` and the decoders' per-step `dh_ext` [T,B,Hp] are __bf16 buffers of the same shapes
     (half the bytes of every time step; the cell state `cs`, dc_ext, the encoders' dh_ext [B, ld_dh], h_init and
     d_h_init stay fp32).  The recurrent product rounds h_{t-1} / dA_t to bf16 anyway, so what is stored is exactly
     what the MFMA consumed; the x-projection and the saved gate activations are rounded once more (nearest even). */
  int32_t store_bf16;
  int32_t bf16_dot;      /* ABI 3, fp32 entry points, forward, small batches (one-row workgroups): the recurrent product runs on
                            bf16 dot products (v_dot2c_f32_bf16; W and h_{t-1} rounded to bf16, fp32 accumulation) -- the small-batch
                            counterpart of the bf16 entry points.  Honoured when every LSTM of the call sets it and the launcher
                            has the variant (the decoders of the canonical sizes); otherwise the fp32 product runs. */
  float* h_last;         /* optional [B, Hp] fp32: forward also writes h_{T-1} here (the latent stack's input stays fp32) */
} MfmSeqDesc;

int mfm_lstm_seq_fwd(const MfmSeqDesc* descs /*host*/, int count, int T, int B, void* stream);

/* bf16 variants: W (rounded once per launch; the decoder's W_ih + W_hh summed in fp32 first), h_{t-1} and dA_t
 * enter v_mfma_f32_16x16x32_bf16 as bf16, accumulation / gate math / cell state / every saved tensor stay fp32.
 * One kernel family for all batch sizes (csrc/lstm_seq_bf16.hip); h > 128 falls back to the fp32 step-by-step path. */
int64_t mfm_lstm_pack_bytes(int32_t h, int32_t is_dec);
int mfm_lstm_pack_bf16(const MfmSeqDesc* descs /*host*/, int count, void* stream);
int mfm_lstm_seq_fwd_bf16(const MfmSeqDesc* descs /*host*/, int count, int T, int B, void* stream);
int mfm_lstm_seq_bwd_bf16(const MfmSeqDesc* descs /*host*/, int count, int T, int B, void* stream);

/* BPTT over the saved gates/cs (autograd of the loops above).  On return `gates` holds the
 * pre-activation gate gradients dA[T,B,4,Hp] (in place); weight/bias gradients are then plain
 * GEMMs over dA (see plan.hip).  For decoders d_h_init receives dA_0 W_ih. */
int mfm_lstm_seq_bwd(const MfmSeqDesc* descs /*host*/, int count, int T, int B, void* stream);

/* ------------------------------------------------------------------------------------------
 * bf16-RESIDENT plans: all weight gradients of ONE LSTM from bf16 buffers in one pass over the gate gradients
 * (csrc/dw_bf16.hip; what autograd accumulates into weight_ih / weight_hh / bias_ih / bias_hh of an nn.LSTMCell unrolled
 * over T, reference mfm_model.py:56,83,85):
 *   dw_ih [4h, dx] += sum_r dA[r]^T xb[r, :dx]      dw_hh [4h, h] (and dw_hh2) += sum_{r >= shift} dA[r]^T hs[r - shift]
 *   db_ih, db_hh [4h] += sum_r dA[r]
 * dA [rows, 4, Hp] bf16 (pad units zero), xb [rows, ldx] bf16 with ldx >= round_up(dx, 16) (NULL: no input product --
 * the decoders, whose step input is h_{t-1}: pass dw_hh2 = dW_ih), hs [rows, Hp] bf16, shift = B (one time step).
 * Test / tuning entry point; the fused plan builds the same launch for all LSTMs and the decoders' fc1 at once. */
int mfm_dw_bf16_lstm(const void* dA, int32_t rows, int32_t h, const void* xb, int32_t ldx, int32_t dx, const void* hs,
                     int32_t shift, float* dw_ih, float* dw_hh, float* dw_hh2, float* db_ih, float* db_hh, void* stream);
/* The same one pass over fp32 buffers (fp32 plans at large T*B): dA [rows, 4, Hp], hs [rows, Hp] fp32; x is the batch itself,
 * [rows, ldx] fp32, of which columns [xcol0, xcol0 + dx) are this LSTM's input (any dword-aligned column range). */
int mfm_dw_f32_lstm(const float* dA, int32_t rows, int32_t h, const float* x, int32_t ldx, int32_t xcol0, int32_t dx,
                    const float* hs, int32_t shift, float* dw_ih, float* dw_hh, float* dw_hh2, float* db_ih, float* db_hh,
                    void* stream);

/* ------------------------------------------------------------------------------------------
 * Reconstruction loss + gradient, replaces nn.MSELoss over x_hat vs the input slices and its
 * backward (mfm_mosi.py:412,437):  loss_slot += sum((xhat-x)^2) * inv_count (un-weighted mean),
 * dxhat = grad_scale * (xhat - x).  x is a column slice of the [T,B,D] batch (row stride ldx).
 */
int mfm_mse_fwd_bwd(const float* xhat, const float* x, int64_t ldx, int64_t rows, int32_t d,
                    float inv_count, float grad_scale, float* dxhat, float* loss_slot, void* stream);

/* ------------------------------------------------------------------------------------------
 * Memory Fusion Network: the memory recurrence of MFN.forward (reference mfm_model.py:177-181),
 *   gamma_n = sigmoid(gamma_n_fc2(drop(relu(gamma_n_fc1([attended_t, mem])))))  n = 1,2
 *   mem     = gamma1 * mem + gamma2 * cHat_t
 * for all T steps in one launch (one workgroup per batch row).  gamma_n_fc1 is split by columns:
 * a1/a2 hold its attended part INCLUDING the bias for all t (a grouped GEMM over [T*B, .]), w1m/w2m
 * are its memory columns [H_n, M] (row-major, contiguous).  Forward overwrites a1/a2 with the
 * post-relu/dropout activations and saves gamma_n and mem_t; backward turns gam1/gam2 into the
 * pre-sigmoid gradients dz_n in place and writes du_n (gradient wrt a_n's pre-activation, which is also
 * the gradient wrt the precomputed attended part) and dchat.  Weight gradients are outer-product sums
 * of these tensors (grouped GEMMs, factorized_amd/mfm_model.py).
 * Returns MFM_ERR_UNSUPPORTED when M / H_n do not fit the register-resident layout. */
typedef struct MfmMemDesc {
  float* a1; float* a2;                 /* [T,B,H1], [T,B,H2] */
  const float* chat;                    /* [T,B,M] */
  const float* w1m; const float* w2m;   /* [H1,M], [H2,M] */
  const float* w1b; const float* b1b;   /* gamma1_fc2: [M,H1], [M] */
  const float* w2b; const float* b2b;   /* gamma2_fc2: [M,H2], [M] */
  float* gam1; float* gam2; float* mems;   /* [T,B,M] each */
  float* mem_out;                       /* [B,M] last memory (forward) */
  const float* dmem_out;                /* [B,M] dL/d mem_T (backward) */
  float* du1; float* du2; float* dchat; /* backward outputs [T,B,H1], [T,B,H2], [T,B,M] */
  int32_t T, B, M, H1, H2, train;
  float p1, p2;                         /* dropout probabilities of gamma1/gamma2 */
  uint64_t seed;
  const uint64_t* seed_dev;             /* optional device word added to `seed` when the kernel runs: lets a captured
                                           hipGraph draw new masks on every replay (the caller advances it in-graph) */
  int64_t ld_wm;                        /* row stride of w1m / w2m (0 = M): lets them be the memory COLUMNS of the
                                           reference's gamma_n_fc1.weight [H_n, att+M] in place, without a copy */
  int32_t dchat_pre_tanh;               /* backward: write dchat * (1 - chat^2), the gradient wrt the PRE-activation of
                                           cHat = tanh(.) (chat then holds the tanh output), instead of dL/dchat */
  int32_t reserved_;
} MfmMemDesc;

int mfm_mfn_mem_fwd(const MfmMemDesc* desc /*host*/, void* stream);
int mfm_mfn_mem_bwd(const MfmMemDesc* desc /*host*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * MMD regulariser of the non-KL MFM, replaces loss_MMD / compute_kernel (reference mfm_model.py:14-34):
 *   *loss += mean K(g,g) + mean K(z,z) - 2 mean K(g,z),  K(a,b) = exp(-mean((a-b)^2)/dim)
 * z, gauss [B, dim] contiguous (the reference draws gauss ~ N(0,1) on the host; the caller supplies it);
 * dz (optional) receives d mmd / d z.  dim <= 256. */
int mfm_mmd_fwd_bwd(const float* z, const float* gauss, int32_t B, int32_t dim, float* loss /*accumulated*/,
                    float* dz /*[B,dim] or NULL*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused Adam on one flat parameter buffer (torch.optim.Adam defaults semantics,
 * mfm_mosi.py:403,441): m,v,p updated in place; g is multiplied by grad_scale first (DP
 * averaging).  `step` is the 1-based step count used for bias correction.
 */
int mfm_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, int32_t step, float lr,
                  float beta1, float beta2, float eps, float grad_scale, void* stream);

/* The same update restricted to up to MFM_ADAM_MAX_SPANS disjoint element ranges of the flat buffer, each with its
 * own 1-based step count; elements outside every span keep p, m and v untouched.  This is torch.optim.Adam's
 * treatment of parameters whose .grad is None (skipped; per-parameter step counters), which staged training
 * relies on: train_beta_vae (reference mfm_mosi.py:278-281, 346-358) trains gen+reg first -- the classifier gets no
 * gradient -- then disc+reg -- the decoders and the modality z->f MLPs get none.  begin/end are multiples of 4.
 * The spans may come in any order; spans that overlap are refused (MFM_ERR_ARG), as are more than MFM_ADAM_MAX_SPANS.  Every
 * span computes the bits mfm_adam_flat computes. */
/* Guarded forms (ABI 3): `guard` is an optional device pointer to ONE float -- by convention a spare element of the gradient
 * buffer itself, so that it travels through the data-parallel all-reduce with the gradients.  The kernels read it first and
 * leave p, m and v untouched unless it is exactly 0.0f.  The fused plan stores a NaN there when an in-launch hand-over of the
 * step gave up waiting (plan option "grad_guard_offset", below): a step whose gradients cannot be trusted does not reach the
 * parameters.  guard == NULL: the unguarded update above. */
int mfm_adam_flat_guarded(float* p, const float* g, float* m, float* v, int64_t n, int32_t step, float lr,
                          float beta1, float beta2, float eps, float grad_scale, const float* guard, void* stream);

/* Capturable form (ABI 3): the 0-based count of updates applied so far and the learning rate live in device memory
 * (`step_dev`, `lr_dev`); the bias corrections are formed on the device and a one-thread launch behind the update advances the
 * counter (not when the guard skipped the step).  This is what a hipGraph of a whole training step replays: kernel arguments
 * are frozen at capture, device words are not (torch.optim.Adam(capturable=True) semantics).  n: a multiple of 4. */
int mfm_adam_flat_dev(float* p, const float* g, float* m, float* v, int64_t n, int32_t* step_dev, const float* lr_dev,
                      float beta1, float beta2, float eps, float grad_scale, const float* guard, void* stream);

#define MFM_ADAM_MAX_SPANS 8
typedef struct MfmAdamSpan { int64_t begin, end; int32_t step; int32_t reserved; } MfmAdamSpan;
int mfm_adam_flat_spans(float* p, const float* g, float* m, float* v, const MfmAdamSpan* spans /*host*/, int32_t nspans,
                        float lr, float beta1, float beta2, float eps, float grad_scale, void* stream);
int mfm_adam_flat_spans_guarded(float* p, const float* g, float* m, float* v, const MfmAdamSpan* spans /*host*/, int32_t nspans,
                                float lr, float beta1, float beta2, float eps, float grad_scale, const float* guard, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused momentum SGD on one flat parameter buffer (torch.optim.SGD semantics, the reference's commented-out optimizer line
 * mfm_mosi.py:404): p and the momentum buffer `buf` updated in place over up to MFM_SGD_MAX_SPANS disjoint element ranges,
 * given in ascending order; elements outside every span keep p and buf untouched (torch skips a parameter whose .grad is
 * None; several parameter groups give one model several sets of hyper-parameters).  Per element of a span:
 *   d = g * grad_scale;  maximize: d = -d;  d += weight_decay * p
 *   momentum != 0:  buf = FIRST ? d : momentum * buf + (1 - dampening) * d;   d = NESTEROV ? d + momentum * buf : buf
 *   p -= lr * d
 * A span with momentum 0 neither reads nor writes buf (buf may be NULL when no span has momentum); FIRST is the step that
 * creates a tensor's buffer (torch: a clone of d), its old contents are not read.  begin/end are multiples of 4; lr,
 * weight_decay and momentum >= 0.  `guard`: as for mfm_adam_flat_guarded (NULL in the unguarded form). */
#define MFM_SGD_MAX_SPANS 112
#define MFM_SGD_NESTEROV 1
#define MFM_SGD_MAXIMIZE 2
#define MFM_SGD_FIRST 4
typedef struct MfmSgdSpan {
  int64_t begin, end;
  float lr, weight_decay, momentum, dampening;
  int32_t flags; /* MFM_SGD_NESTEROV | MFM_SGD_MAXIMIZE | MFM_SGD_FIRST */
  int32_t reserved;
} MfmSgdSpan;
int mfm_sgd_flat_spans(float* p, const float* g, float* buf, const MfmSgdSpan* spans /*host*/, int32_t nspans, float grad_scale,
                       void* stream);
int mfm_sgd_flat_spans_guarded(float* p, const float* g, float* buf, const MfmSgdSpan* spans /*host*/, int32_t nspans,
                               float grad_scale, const float* guard, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused Adam with every option of torch.optim.Adam / AdamW (weight decay, decoupled decay, AMSGrad, maximize) on one flat
 * parameter buffer: p, the moments m and v and the running maximum vmax updated in place over up to MFM_ADAMX_MAX_SPANS
 * disjoint element ranges, given in ascending order, each with its own hyper-parameters and 1-based step count; elements
 * outside every span keep p, m, v and vmax untouched (torch skips a parameter whose .grad is None; several parameter groups
 * give one model several sets of hyper-parameters).  Per element of a span, in the order of torch's _single_tensor_adam:
 *   d = g * grad_scale;  MAXIMIZE: d = -d
 *   weight_decay != 0:  DECOUPLED ? p *= 1 - lr * weight_decay  :  d += weight_decay * p
 *   m += (1 - beta1) * (d - m);   v = beta2 * v + (1 - beta2) * d * d
 *   AMSGRAD: vmax = max(vmax, v);   denom = sqrt(AMSGRAD ? vmax : v) / sqrt(1 - beta2^step) + eps
 *   p -= lr / (1 - beta1^step) * m / denom
 * A span without AMSGRAD neither reads nor writes vmax (vmax may be NULL when no span has the flag).  A span with no flag and
 * weight_decay 0 computes what mfm_adam_flat computes.  begin/end are multiples of 4; lr, eps and weight_decay >= 0;
 * 0 <= beta < 1; step >= 1.  `guard`: as for mfm_adam_flat_guarded (NULL in the unguarded form). */
#define MFM_ADAMX_MAX_SPANS 88
#define MFM_ADAMX_MAXIMIZE 1
#define MFM_ADAMX_AMSGRAD 2
#define MFM_ADAMX_DECOUPLED 4
typedef struct MfmAdamExtSpan {
  int64_t begin, end;
  int32_t step;  /* 1-based count of updates of this span, this one included */
  int32_t flags; /* MFM_ADAMX_MAXIMIZE | MFM_ADAMX_AMSGRAD | MFM_ADAMX_DECOUPLED */
  float lr, beta1, beta2, eps, weight_decay;
  int32_t reserved;
} MfmAdamExtSpan;
int mfm_adam_ext_flat_spans(float* p, const float* g, float* m, float* v, float* vmax, const MfmAdamExtSpan* spans /*host*/,
                            int32_t nspans, float grad_scale, void* stream);
int mfm_adam_ext_flat_spans_guarded(float* p, const float* g, float* m, float* v, float* vmax,
                                    const MfmAdamExtSpan* spans /*host*/, int32_t nspans, float grad_scale, const float* guard,
                                    void* stream);

/* ------------------------------------------------------------------------------------------
 * Gradient clipping on one flat gradient buffer (torch.nn.utils.clip_grad_norm_ / clip_grad_value_ semantics;
 * factorized_amd.nn_utils): g changed in place over up to MFM_CLIP_MAX_SPANS disjoint element ranges, given in ascending order;
 * elements outside every span are neither read into a norm nor written (torch skips a parameter whose .grad is None, and
 * the padding behind a tensor of the flat layout keeps its bits).  begin is a multiple of 4, end is ANY element index above
 * it: a span is a tensor's exact extent.
 *   norm:   total_norm = ||g over the spans|| of kind MFM_NORM_L2 / MFM_NORM_INF / MFM_NORM_L1 (the max propagates a NaN);
 *           g *= min(max_norm / (total_norm + 1e-6), 1), always multiplied, a NaN coefficient stays NaN (as torch, in fp32).
 *           Two launches on `stream`, no atomics: the same table gives the same bits.  `ws` holds
 *           mfm_clip_workspace_floats() floats of scratch; total_norm is one device float.
 *   value:  g = clamp(g, -clip_value, clip_value), a NaN stays NaN; one launch.
 * max_norm and clip_value >= 0.  `guard`: optional device float; if it is anything but 0.0f, g is left untouched and
 * total_norm is NaN (gradients that cannot be trusted are not rescaled and report no finite norm); NULL: unguarded. */
#define MFM_CLIP_MAX_SPANS 112 /* >= 104: every tensor of MFM_KL as its own span */
#define MFM_NORM_L2 0
#define MFM_NORM_INF 1
#define MFM_NORM_L1 2
typedef struct MfmClipSpan {
  int64_t begin, end; /* begin % 4 == 0, end > begin */
} MfmClipSpan;
int64_t mfm_clip_workspace_floats(void); /* host only: floats `ws` must hold */
int mfm_clip_grad_norm_flat_spans(float* g, const MfmClipSpan* spans /*host*/, int32_t nspans, int32_t norm_kind, float max_norm,
                                  float* ws, float* total_norm /*device, 1 float*/, const float* guard, void* stream);
int mfm_clip_grad_value_flat_spans(float* g, const MfmClipSpan* spans /*host*/, int32_t nspans, float clip_value,
                                   const float* guard, void* stream);

/* ------------------------------------------------------------------------------------------
 * Decoder output layers, forward and backward to the hidden states, for up to 3 decoders in ONE launch (the launch the
 * fp32 plans run between the decoder recurrence and its BPTT; csrc/dec_fc1.hip).  Per item, over `rows` rows:
 *   x_hat = H Wfc^T + b;  diff = x_hat - x;  *loss += sum(diff^2) * inv_count;  dx_hat = grad_scale * diff;
 *   with_bwd:  dH = dx_hat Wfc, units [h, Hp) of every row written as zeros
 * H [rows, Hp] with units [h, Hp) zero, Hp a multiple of 16; Wfc [d, h]; x row stride ldx; xhat / dxhat [rows, d] optional.
 * bf16_operands: H, Wfc and dx_hat are rounded to bf16 (RNE) on their way into the products (fp32 accumulation).
 * d <= 128: dH is stored (same bits every time).  d > 128: the column groups ADD into dH, the caller clears it first and says
 * so with dhs_zeroed.  Returns MFM_ERR_UNSUPPORTED (no error text, nothing launched) for Hp > 128, for d * h >= 2^28 and for
 * d > 128 with with_bwd and without dhs_zeroed. */
typedef struct MfmDecFc1Item {
  const float* hs; const float* w; const float* bias; const float* x;
  float* xhat; float* dxhat; float* dhs; float* loss;
  int64_t ldx;
  int32_t d, h, Hp;
  float inv_count, grad_scale;
  int32_t pad_;
} MfmDecFc1Item;
int mfm_dec_fc1_f32(const MfmDecFc1Item* items /*host*/, int32_t count, int32_t rows, int32_t with_bwd, int32_t bf16_operands,
                    int32_t dhs_zeroed, void* stream);

/* ------------------------------------------------------------------------------------------
 * Weight averaging of one flat parameter buffer into another of the same layout (torch.optim.swa_utils.AveragedModel
 * semantics; factorized_amd.swa_utils): one launch over the element range [begin, end), nothing outside it is read or written
 * in either buffer, p is never written.  The update count n is read from device memory (`n_averaged`: the int64 word of
 * AveragedModel.n_averaged), never from the host:
 *   n == 0:  avg = p, bit for bit (NaN payloads and infinities included), whatever the kind
 *   n  > 0:  avg = lerp(avg, p, w) by torch's rule:  |w| < 0.5 ? avg + w * (p - avg) : p - (p - avg) * (1 - w)
 *            MFM_AVG_SWA: w = 1.0f / (float)(n + 1) (the argument `w` is ignored);  MFM_AVG_EMA: w as passed, 1 - decay in [0, 1]
 * and the launch stores n + 1 back itself (a captured launch advances the count on every replay): every workgroup reads n
 * first and draws a ticket from `ticket` when it is done; the last one stores n + 1 and sets the ticket word back to 0.
 * `ticket` is one device int32 that holds 0 between launches and is used by one launch at a time.  begin/end are multiples
 * of 4, avg and p 16-byte aligned, n_averaged 8-byte aligned. */
#define MFM_AVG_SWA 0
#define MFM_AVG_EMA 1
int mfm_avg_flat(float* avg, const float* p, int64_t begin, int64_t end, int32_t kind, float w, int64_t* n_averaged /*device*/,
                 int32_t* ticket /*device, zero between launches*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * Keep the best weights (factorized_amd.checkpoint.KeepBest; the reference's `if valid_loss <= best_valid: ... torch.save(model)`):
 * one launch compares a metric with state->best_value and, if it is at least as good, copies the element range [begin, end)
 * of the live flat parameter buffer `p` into the snapshot `best` of the same layout, bit for bit; nothing outside the range is
 * read or written in either buffer, p is never written, and a launch that does not take moves no parameter byte at all.
 *   MFM_KEEP_MIN: take = metric <= best_value      MFM_KEEP_MAX: take = metric >= best_value
 * (a tie takes the newer weights; a NaN metric never takes; the comparison is in fp32).  The metric is the device float
 * `metric_dev` points to or, when that is NULL, the argument `metric`.  The launch updates the state itself (a captured launch
 * decides anew on every replay): taken -> best_value = metric, best_call = calls; always taken = 0 | 1 and calls += 1.  Every
 * workgroup reads the state first and draws a ticket from state->ticket when it is done; the last one stores the new state and
 * sets the ticket word back to 0.  The caller initialises the block (best_value = +inf / -inf or a bound such as the
 * reference's 999999.0, calls = 0, best_call = -1, taken = 0, ticket = 0); one launch at a time may use it.  begin/end are
 * multiples of 4, best and p 16-byte aligned, state 16-byte aligned, metric_dev 4-byte aligned. */
#define MFM_KEEP_MIN 0
#define MFM_KEEP_MAX 1
typedef struct MfmKeepBestState {
  float best_value;
  int32_t calls;     /* launches so far */
  int32_t best_call; /* 0-based index of the launch that last took a snapshot, -1: none yet */
  int32_t taken;     /* 1: the latest launch took a snapshot */
  int32_t ticket;    /* 0 between launches */
  int32_t reserved_[3];
} MfmKeepBestState;
int mfm_keep_best_flat(float* best, const float* p, int64_t begin, int64_t end, int32_t mode, const float* metric_dev /*device or NULL*/,
                       float metric, MfmKeepBestState* state /*device*/, void* stream);

/* ------------------------------------------------------------------------------------------
 * Reduce the learning rate on a plateau (factorized_amd.lr_scheduler.ReduceLROnPlateau; the reference's `scheduler.step(valid_loss)`
 * with torch.optim.lr_scheduler.ReduceLROnPlateau at the end of every epoch): one launch of one wave, one working lane, reads
 * a metric, advances *state and, when the rule says so, scales the fp32 learning-rate words of n_groups parameter groups in
 * device memory.  The rule is torch 2.10's step / _is_better / _reduce_lr in fp64, statement for statement and without
 * contraction, so state and lr bits equal torch's on the same inputs:
 *   current = (double)metric;  last_epoch = epoch == -1 ? last_epoch + 1 : epoch
 *   better:  MIN/REL current < best * (1 - threshold)   MIN/ABS current < best - threshold
 *            MAX/REL current > best * (threshold + 1)   MAX/ABS current > best + threshold       (false for a NaN metric)
 *   better ? (best = current, num_bad_epochs = 0) : num_bad_epochs += 1
 *   cooldown_counter > 0 ?  cooldown_counter -= 1, num_bad_epochs = 0
 *   num_bad_epochs > patience ?  for every group, in order:  old = (double)*lr;  new = max(old * factor, min_lr);
 *                                                            if (old - new > eps) *lr = (float)new
 *                                then cooldown_counter = cooldown, num_bad_epochs = 0
 *   reduced = 1 if an lr word was stored, else 0;  reductions += reduced
 * The metric is the device float `metric_dev` points to or, when that is NULL, the argument `metric` (a double: a host value
 * keeps its precision).  Groups that share one lr word are reduced once per group, as by torch's loop; a launch that does not
 * reduce stores no lr word.  The caller initialises the block (best = +inf for MIN, -inf for MAX, everything else 0); one launch
 * at a time may use it.  state is 16-byte aligned, metric_dev and every lr pointer 4-byte aligned; 1 <= n_groups <=
 * MFM_PLATEAU_MAX_GROUPS; factor < 1; patience, cooldown >= 0.  Stream-ordered, no host synchronisation, legal inside a stream
 * capture (the scalar arguments and the table are then part of the graph; the decision is taken anew on every replay). */
#define MFM_PLATEAU_MAX_GROUPS 16
#define MFM_PLATEAU_MIN 0
#define MFM_PLATEAU_MAX 1
#define MFM_PLATEAU_REL 0
#define MFM_PLATEAU_ABS 1
typedef struct MfmPlateauState {
  double best;
  int32_t num_bad_epochs;
  int32_t cooldown_counter;
  int32_t last_epoch;
  int32_t reduced;    /* 1: the latest launch changed at least one lr */
  int32_t reductions; /* launches so far that did */
  int32_t reserved_;
} MfmPlateauState;
typedef struct MfmPlateauGroups {
  float* lr[MFM_PLATEAU_MAX_GROUPS]; /* device, one fp32 word per group */
  double min_lr[MFM_PLATEAU_MAX_GROUPS];
} MfmPlateauGroups;
int mfm_plateau_step(MfmPlateauState* state /*device*/, const float* metric_dev /*device or NULL*/, double metric,
                     const MfmPlateauGroups* groups /*host*/, int32_t n_groups, int32_t mode, int32_t threshold_mode, double factor,
                     double threshold, double eps, int32_t patience, int32_t cooldown, int32_t epoch /*-1: last_epoch + 1*/,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * Reshuffle of a device-resident split (factorized_amd.train.DeviceDataset.reshuffle): one launch gathers the samples of a
 * sample-major pool through a device permutation into the batch layout the plans consume, for b < nb, t < T, r < B:
 *   X[b, t, r, :] = X_pool[perm[b * B + r], t, :]         X [nb, T, B, D] fp32,  X_pool [N, T, D] fp32
 *   y[b, r, :]    = y_pool[perm[b * B + r], :]            label rows of `ybytes` opaque bytes each (a multiple of 4:
 *                                                         float [N], float [N, k], int64 [N], ...)
 * `perm` is a DEVICE array of N int64 indices (what torch.randperm and torch indexing use); only its first nb * B entries
 * are read, the rest are the samples this epoch leaves out.  A pure copy: every bit arrives unchanged, nothing outside
 * the nb * T * B * D floats of X and the nb * B * ybytes bytes of y is written, the pool is never written.  An index outside
 * [0, N) is skipped (its rows of X and y keep their bytes); a repeated index is copied twice: whether perm is a permutation
 * is the caller's to check.  No constraint on D or B; rows move in 16-byte accesses when D % 4 == 0 and X and X_pool are
 * 16-byte aligned, in dwords otherwise.  nb * B <= N, nb * T * B < 2^31, all buffers 4-byte aligned, perm 8-byte aligned,
 * batches and pool disjoint.  Stream-ordered, no host synchronisation, legal inside a stream capture. */
int mfm_dataset_gather(float* X, void* y, const float* X_pool, const void* y_pool, const int64_t* perm /*device, N*/, int64_t N,
                       int32_t nb, int32_t T, int32_t B, int32_t D, int64_t ybytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Prediction-only path of MFM_KL_EF (csrc/predict.hip): `evaluate(model, X, y)` / `predict(model, X)` of the reference's
 * drivers (mfm_mosi.py:445-477), which use y_hat alone.  In eval mode y_hat depends on ONE of the model's seven recurrences
 * (mfm_model.py:637-657):
 *   ef_last = ef_encoder(x); zy = last_to_zy_fc1(ef_last); fy = relu(zy_to_fy_fc2(relu(zy_to_fy_fc1(zy))));
 *   y_hat = fy_to_y_fc2(relu(fy_to_y_fc1(fy)))
 * so this entry runs the ef encoder's input projection (grouped fp32 GEMM) and ONE further launch per row chunk: the T-step
 * recurrence with h / c on chip -- no hs / cs / gate record is stored -- and the six row-wise layers behind it in the same
 * workgroup.  It needs no MfmPlan and no training workspace.  fp32.
 *   sizes    x [T, N, D] time-major and contiguous (4-byte aligned: any contiguous view); h = hidden size of the ef encoder
 *            (zl + za + zv); zy, fy, output_dim
 *   params   base of the flat fp32 parameter buffer; `offsets` (host, 16 element offsets into it): ef_encoder.lstm
 *            weight_ih, weight_hh, bias_ih, bias_hh, then weight and bias of ef_encoder.fc1, last_to_zy_fc1, zy_to_fy_fc1,
 *            zy_to_fy_fc2, fy_to_y_fc1, fy_to_y_fc2 (torch layouts; the two LSTM weights 16-byte aligned)
 *   y        NULL, or the labels: float [N, output_dim] (loss_kind 0, L1) / int64 [N] (loss_kind 1, cross entropy)
 *   y_hat    out [N, output_dim]
 *   loss_dev NULL, or one device float that receives the mean nn.L1Loss() / nn.CrossEntropyLoss() would give (needs y).
 *            One partial per workgroup and a last-arriver ticket that adds the partials in a fixed order: no float atomics,
 *            the value is bit-identical from run to run; the ticket word is cleared by the call itself and left at 0.
 *   max_rows row cap: the split is walked in chunks of at most max_rows rows (0: one chunk) that share the workspace; the
 *            loss is the mean over all N rows whatever the chunking
 *   workspace mfm_predict_klef_workspace_floats(T, N, h, max_rows) floats, 16-byte aligned, contents arbitrary:
 *            min(N, max_rows) * T * 4 * round_up(h, 16) for the x-projections + N loss partials + 4
 * Nothing outside workspace, y_hat and *loss_dev is written.  Any N >= 1, T >= 1.  Sizes the on-chip recurrence does not cover
 * (h > 128, or more LDS than a CU has) return MFM_ERR_UNSUPPORTED with the size in the error text and enqueue nothing: run
 * mfm_plan_forward(train = 0) instead.  Stream-ordered, no host synchronisation, legal inside a stream capture. */
int64_t mfm_predict_klef_workspace_floats(int32_t T, int64_t N, int32_t h, int64_t max_rows); /* host only; 0 for bad sizes */
int mfm_predict_klef(int32_t T, int64_t N, int32_t D, int32_t h, int32_t zy, int32_t fy, int32_t output_dim, int32_t loss_kind,
                     const float* params, const int64_t* offsets /*host, 16*/, const float* x, const void* y /*or NULL*/,
                     float* workspace, float* y_hat, float* loss_dev /*or NULL*/, int64_t max_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * The factorized latents and generation from them (csrc/generate.hip): the two halves of the eval-mode forward
 * (mfm_model.py:619-660) as calls of their own, in the pattern of mfm_predict_klef -- recurrences with h / c on chip, the
 * row-wise layers in the same workgroup, no MfmPlan and no training workspace, nothing a backward would read is stored.  fp32;
 * dropout is the identity and the means are used (no sampling).
 *
 * mfm_encode_klef: the encoder half of MFM_KL_EF (mfm_model.py:627-639),
 *   z_m = last_to_z{m}_fc1(encoder_m(x_m)), logvar_z_m = last_to_logvarz{m}_fc1(encoder_m(x_m)) for m = l, a, v on the column
 *   ranges [0, d_l), [d_l, d_l + d_a), [d_l + d_a, D) of x, and zy / logvar_zy likewise from ef_encoder(x).
 * Per row chunk: the four input projections as one grouped fp32 GEMM, then ONE launch whose workgroups are (encoder, row
 * tile): the T-step recurrence, then the encoder's fc1, the mean head and the logvar head on the tile's last hidden states.
 *   sizes    x [T, N, D] time-major and contiguous (4-byte aligned: any contiguous view), D = d_l + d_a + d_v; hidden sizes
 *            zl, za, zv and zl + za + zv; zy
 *   params   base of the flat fp32 parameter buffer; `offsets` (host, 40 element offsets into it), per encoder in the order
 *            encoder_l, encoder_a, encoder_v, ef_encoder: lstm weight_ih, weight_hh, bias_ih, bias_hh, fc1 weight, bias, then
 *            weight and bias of its mean head (last_to_zl / za / zv / zy _fc1) and of its logvar head (torch layouts; the LSTM
 *            weights 16-byte aligned)
 *   out      host array of 8 device pointers: zl [N, zl], za [N, za], zv [N, zv], zy [N, zy], then the four logvars alike
 *   max_rows row cap: chunks of at most max_rows rows (0: one chunk) that share the workspace
 *   workspace mfm_encode_klef_workspace_floats(T, N, zl, za, zv, max_rows) floats, 16-byte aligned, contents arbitrary:
 *            min(N, max_rows) * T * 4 * (round_up(zl, 16) + round_up(za, 16) + round_up(zv, 16) + round_up(zl + za + zv, 16))
 *
 * mfm_decode_factors: the generative half, identical in MFM_KL_EF, MFM_KL and MFM (mfm_model.py:644-657),
 *   fy = relu(zy_to_fy_fc2(relu(zy_to_fy_fc1(zy)))), f_m likewise from z_m; x_m_hat = decoder_m(cat([fy, f_m]), T);
 *   y_hat = fy_to_y_fc2(relu(fy_to_y_fc1(fy)))
 * The four factors are independent inputs with N rows each.  Per row chunk: ONE launch whose workgroups are (decoder, row
 * tile) -- fy and f_m of the tile's rows into LDS (the three decoders' workgroups recompute fy on the same code path:
 * bit-identical), the decoder recurrence from there (step 0: W_ih on the embedding, then W_ih + W_hh on h) storing h_t alone,
 * decoder l's workgroups also the classifier and y_hat -- then the three decoders' fc1 as one grouped fp32 GEMM into x_m_hat.
 *   sizes    host, 12: zl, za, zv, zy, fl, fa, fv, fy, d_l, d_a, d_v, output_dim (decoder m has hidden size fy + f_m)
 *   offsets  host, 38 element offsets: weight and bias of zy_to_fy_fc1, zy_to_fy_fc2, zl_to_fl_fc1, zl_to_fl_fc2, za_to_fa_fc1,
 *            za_to_fa_fc2, zv_to_fv_fc1, zv_to_fv_fc2; per decoder (l, a, v) lstm weight_ih, weight_hh, bias_ih, bias_hh, fc1
 *            weight, bias; weight and bias of fy_to_y_fc1, fy_to_y_fc2 (the LSTM weights 16-byte aligned)
 *   z        host array of 4 device pointers: zl [N, zl], za [N, za], zv [N, zv], zy [N, zy], contiguous, 4-byte aligned each
 *   out      host array of 4 device pointers: x_l_hat [T, N, d_l], x_a_hat [T, N, d_a], x_v_hat [T, N, d_v], y_hat [N, output_dim]
 *   workspace mfm_decode_factors_workspace_floats(T, N, fy, fl, fa, fv, max_rows) floats, 16-byte aligned, contents arbitrary:
 *            min(N, max_rows) * T * (round_up(fy + fl, 16) + round_up(fy + fa, 16) + round_up(fy + fv, 16)) for the stored h
 *
 * Both: nothing outside the workspace and the outputs is written.  Any N >= 1, T >= 1.  Sizes the on-chip recurrence does not
 * cover (a hidden size > 128, or more LDS than a CU has) return MFM_ERR_UNSUPPORTED with the size in the error text and enqueue
 * nothing: compose the granular entries instead.  Stream-ordered, no host synchronisation, legal inside a stream capture. */
int64_t mfm_encode_klef_workspace_floats(int32_t T, int64_t N, int32_t zl, int32_t za, int32_t zv, int64_t max_rows); /* host only; 0 for bad sizes */
int mfm_encode_klef(int32_t T, int64_t N, int32_t d_l, int32_t d_a, int32_t d_v, int32_t zl, int32_t za, int32_t zv, int32_t zy,
                    const float* params, const int64_t* offsets /*host, 40*/, const float* x, float* workspace,
                    float* const* out /*host, 8*/, int64_t max_rows, void* stream);
int64_t mfm_decode_factors_workspace_floats(int32_t T, int64_t N, int32_t fy, int32_t fl, int32_t fa, int32_t fv,
                                            int64_t max_rows); /* host only; 0 for bad sizes */
int mfm_decode_factors(int32_t T, int64_t N, const int32_t* sizes /*host, 12*/, const float* params, const int64_t* offsets /*host, 38*/,
                       const float* const* z /*host, 4*/, float* workspace, float* const* out /*host, 4*/, int64_t max_rows,
                       void* stream);

/* ------------------------------------------------------------------------------------------
 * mfm_encode_mfn (csrc/encode_mfn.hip): the encoder half of MFM_KL and MFM, whose label factor comes from the Memory Fusion
 * Network (mfm_model.py:140-199, :723-743), in the pattern and under the contract of mfm_encode_klef: fp32, dropout the
 * identity, the means used, no MfmPlan and no training workspace.
 *   m_last = encoder_m(x_m) (the recurrence, then the encoder's fc1) for m = l, a, v.  heads = 1 (MFM_KL): z_m =
 *   last_to_z{m}_fc1(m_last), logvar_z_m = last_to_logvarz{m}_fc1(m_last).  heads = 0 (MFM): z_m = m_last, no logvars.
 *   MFN: the three LSTMCell recurrences on x_l, x_a, x_v; cStar_t = [c_{t-1} | c_t], c_{-1} = 0; attended = softmax(att1_fc2(
 *   relu(att1_fc1(cStar)))) * cStar; cHat = tanh(att2_fc2(relu(att2_fc1(attended)))); gamma_g = sigmoid(gamma{g}_fc2(relu(
 *   gamma{g}_fc1([attended | mem])))); mem = gamma1 * mem + gamma2 * cHat; zy = last_to_zy_fc1([h_l,T | h_a,T | h_v,T | mem_T])
 *   and, heads = 1, logvar_zy = last_to_logvarzy_fc1 of the same.  The MFN's out_fc* layers are not used, as in the reference.
 * Per row chunk four launches behind one grouped fp32 GEMM for the six input projections: the six recurrences as (LSTM, row
 * tile) workgroups (the encoders with their fc1 and heads; the MFN's LSTMs store their cell states and last hidden state, no h
 * record and no gates); the attention chain row-wise over the T * n pairs (t, row) on the fp32 MFMA with cStar, attention and
 * attended in LDS only -- per pair cHat and the attended part of the two gamma pre-activations are written; the memory
 * recurrence with one workgroup per row, mem on chip, ending with the label head(s).
 *   sizes    host, 17: d_l, d_a, d_v; zl, za, zv (the encoders' hidden sizes); zy; h_l, h_a, h_v (h_dims); memsize; windowsize;
 *            the hidden widths of att1, att2, gamma1, gamma2; heads (1: MFM_KL, 0: MFM)
 *   offsets  host, element offsets into the flat fp32 parameter buffer `params`.  Per encoder l, a, v: lstm weight_ih,
 *            weight_hh, bias_ih, bias_hh, fc1 weight, bias and, heads = 1, weight and bias of its mean head and of its logvar
 *            head (10 or 6 each); per MFN LSTM l, a, v: weight_ih, weight_hh, bias_ih, bias_hh (12); weight and bias of att1_fc1,
 *            att1_fc2, att2_fc1, att2_fc2, gamma1_fc1, gamma1_fc2, gamma2_fc1, gamma2_fc2 (16); of last_to_zy_fc1 and, heads = 1,
 *            last_to_logvarzy_fc1.  62 offsets with heads, 48 without (torch layouts; the LSTM weights 16-byte aligned)
 *   x        [T, N, D] time-major and contiguous, D = d_l + d_a + d_v, 4-byte aligned: any contiguous view
 *   out      host array of 8 device pointers in the order zl [N, zl], za, zv, zy [N, zy], then the four logvars alike; heads = 0:
 *            the last four are not read and may be NULL
 *   max_rows row cap: chunks of at most max_rows rows (0: one chunk) that share the workspace
 *   workspace mfm_encode_mfn_workspace_floats(T, N, sizes, max_rows) floats, 16-byte aligned, contents arbitrary.  With
 *            rows = min(N, max_rows), Hp(h) = round_up(h, 16), up4(v) = round_up(v, 4):
 *              rows * T * 4 * (Hp(zl) + Hp(za) + Hp(zv) + Hp(h_l) + Hp(h_a) + Hp(h_v))      the x-projections
 *            + rows * T * (Hp(h_l) + Hp(h_a) + Hp(h_v))                                     the MFN LSTMs' cell states
 *            + up4(rows * h_l) + up4(rows * h_a) + up4(rows * h_v)                          their last hidden states
 *            + up4(rows * T * memsize) + up4(rows * T * gamma1) + up4(rows * T * gamma2)    cHat and the gamma partials
 * Determinism: bit-identical from run to run.  The recurrence launch runs on one-row tiles while 6 * rows < 6 * CUs and on
 * four-row tiles from there (mfm_encode_mfn_tile_rows tells which; host only, -1 for bad arguments); the other launches have
 * one form (the attention chain takes 16 or 32 pairs per workgroup, and a pair's arithmetic is the same in both).  For a
 * fixed tile-row form the results are bit-identical for every row chunking.
 * Nothing outside the workspace and the outputs is written.  Any N >= 1, T >= 1.  MFM_ERR_UNSUPPORTED with the size in the
 * error text, nothing enqueued: an h_dims entry or an encoder hidden size above 128; a windowsize other than 2 (the reference's
 * forward reads exactly two steps); attention widths whose tile needs more than the 160 KB of LDS of a CU; memsize or gamma
 * widths beyond the register-resident memory recurrence (more than 1024 threads, or a reduction longer than 512).  Compose
 * the granular entries instead.  Stream-ordered, no host synchronisation, legal inside a stream capture. */
int64_t mfm_encode_mfn_workspace_floats(int32_t T, int64_t N, const int32_t* sizes /*host, 17*/, int64_t max_rows); /* host only; 0 for bad sizes */
int mfm_encode_mfn_tile_rows(int64_t N, int64_t max_rows);
int mfm_encode_mfn(int32_t T, int64_t N, const int32_t* sizes /*host, 17*/, const float* params, const int64_t* offsets /*host, 62 or 48*/,
                   const float* x, float* workspace, float* const* out /*host, 8*/, int64_t max_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * The full validation objective of MFM_KL_EF (csrc/objective.hip; reference mfm_mosi.py:319-324, :724-726, :826-845): the six
 * numbers every driver reports for a validation split, from the deterministic eval forward, in the pattern of the entries
 * above -- fp32, dropout the identity, z = the mean heads, no MfmPlan, no training workspace, and no x_hat in memory.
 *   out[1] disc   mean L1 (loss_kind 0) / cross entropy (1) of y_hat, as mfm_predict_klef defines it
 *   out[2..4] gen_l, gen_a, gen_v   mean over T * N * d_m of (x_m_hat - x_m)^2
 *   out[5] reg    sum over the four factors of -0.5 * sum(1 + logvar - mu^2 - exp(logvar))
 *   out[0] loss   disc + lambdas[0] * gen_l + lambdas[1] * gen_a + lambdas[2] * gen_v + lambdas[3] * reg
 * Per row chunk: the launches of mfm_encode_klef (means and log-variances into the workspace), the recurrence launch of
 * mfm_decode_factors on the means (h_t of the three decoders and y_hat into the workspace), ONE launch of (decoder, 64-row
 * tile, 64-column tile) workgroups that form x_hat = h W_fc1^T + b in registers, subtract the matching slice of x and leave one
 * squared-error partial each, and one single-workgroup launch that adds the chunk's partials, KLD terms and label-loss terms
 * in a fixed order into fp64 accumulators of the workspace; behind the last chunk it divides by the counts of the WHOLE split
 * and writes `out`.  No float atomics: the six values are bit-identical from run to run for a given (T, N, max_rows).
 *   sizes    host, 13: zl, za, zv, zy, fl, fa, fv, fy, d_l, d_a, d_v, output_dim (as mfm_decode_factors), loss_kind
 *   lambdas  host, 4: lda_xl, lda_xa, lda_xv, lda_mmd
 *   offsets  host, 78 element offsets into the flat fp32 parameter buffer `params`: the 40 of mfm_encode_klef, then the 38 of
 *            mfm_decode_factors
 *   x        [T, N, D] time-major and contiguous, D = d_l + d_a + d_v, 4-byte aligned: any contiguous view (a batch of a
 *            resident dataset, a time crop); params and the workspace alone must be on 16 bytes
 *   y        the labels: float [N, output_dim] (loss_kind 0) / int64 [N] (loss_kind 1)
 *   out      6 device floats (4-byte aligned)
 *   max_rows row cap: chunks of at most max_rows rows (0: one chunk) that share the workspace; every mean is over the whole
 *            split whatever the chunking
 *   workspace mfm_objective_klef_workspace_floats(T, N, sizes, max_rows) floats, 16-byte aligned, contents arbitrary; with
 *            rows = min(N, max_rows): the larger of the two entries' workspaces above (the stored h takes the place of the
 *            x-projections), the chunk's eight factors and y_hat, one partial per workgroup of the squared-error launch, and
 *            the accumulators -- it does not grow with N beyond the row cap
 * Nothing outside the workspace and `out` is written.  T < 1, N < 1, a null pointer or max_rows < 0 return MFM_ERR_ARG before
 * anything touches the GPU.  Any N >= 1 (< 2^24), T >= 1.  Sizes the on-chip recurrence does not cover (a hidden size > 128, or more LDS
 * than a CU has) return MFM_ERR_UNSUPPORTED with the size in the error text and enqueue nothing: run mfm_plan_forward(train = 0)
 * instead.  Stream-ordered, no host synchronisation, legal inside a stream capture. */
int64_t mfm_objective_klef_workspace_floats(int32_t T, int64_t N, const int32_t* sizes /*host, 13*/, int64_t max_rows); /* host only; 0 for bad sizes */
int mfm_objective_klef(int32_t T, int64_t N, const int32_t* sizes /*host, 13*/, const float* lambdas /*host, 4*/, const float* params,
                       const int64_t* offsets /*host, 78*/, const float* x, const void* y, float* workspace, float* out /*6*/,
                       int64_t max_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * mfm_objective_mfn (csrc/objective_mfn.hip): the same six numbers, under the same contract, for MFM_KL and MFM, whose label
 * factor comes from the Memory Fusion Network (mfm_model.py:140-199, :723-743).  heads = 1 (MFM_KL): reg as above, over the four
 * (mean, logvar) pairs.  heads = 0 (MFM): the factors are the encoders' fc1 outputs and last_to_zy_fc1, and
 *   out[5] reg    sum over the four factors z [N, dim] of mean K(g, g) + mean K(z, z) - 2 mean K(g, z),
 *                 K(a, b) = exp(-|a - b|^2 / dim^2) (mfm_model.py:14-34), the means over all N^2 pairs of the WHOLE split, g the
 *                 factor's columns of `gauss`
 * Per row chunk of n rows: the launches of mfm_encode_mfn as that entry launches them (the grouped projection GEMM, the six
 * recurrences in one launch, the attention chain, the memory recurrence with the label head(s)), the factors into the workspace
 * -- with heads the chunk's means and log-variances, without heads the means into their rows of four whole-split arrays
 * [N, size]; the recurrence launch of mfm_decode_factors on the chunk's means (the stored h takes the place of the
 * projections); the fused fc1 / squared-error launch and the single-workgroup fp64 finish of mfm_objective_klef.  With heads that
 * finish writes `out` behind the last chunk.  Without heads two more launches follow the last chunk: the MMD, value only --
 * workgroup (factor, tile of 8 rows i for N <= 256, else 32) walks j in tiles of 32 rows staged in LDS, forms the three kernel
 * values per pair with expf, adds kzz + kgg - 2 kgz per pair, reduces lane -> wave -> workgroup in a fixed order and writes ONE
 * partial to its own slot -- and a finish that adds each factor's partials in ascending order in fp64, scales by 1 / N^2, forms
 * the total and writes `out`.  No gradient, no [N, N] scratch, no float atomics.
 *   sizes    host, 23: as mfm_predict_zeros_mfn (entry 16, heads, tells MFM_KL from MFM)
 *   lambdas  host, 4: lda_xl, lda_xa, lda_xv, lda_mmd
 *   offsets  host, 100 (heads = 1) or 86 (heads = 0): as mfm_predict_zeros_mfn (with heads the logvar heads' are read here)
 *   x, y, out, max_rows   as mfm_objective_klef
 *   gauss    heads = 0: the N(0, 1) sample, [N, zl + za + zv + zy] contiguous (columns in that order), 4-byte aligned, read
 *            only; heads = 1: must be NULL.  Either the other way round is MFM_ERR_ARG
 *   workspace mfm_objective_mfn_workspace_floats(T, N, sizes, max_rows) floats, 16-byte aligned, contents arbitrary.  With
 *            rows = min(N, max_rows), Hp(h) = round_up(h, 16), up4(v) = round_up(v, 4):
 *              max(rows * T * 4 * (Hp(zl) + Hp(za) + Hp(zv) + Hp(h_l) + Hp(h_a) + Hp(h_v)),   the six x-projections, and in their
 *                  rows * T * (Hp(fy + fl) + Hp(fy + fa) + Hp(fy + fv)))                      place the decoders' stored h
 *            + rows * T * (Hp(h_l) + Hp(h_a) + Hp(h_v))                                       the MFN LSTMs' cell states
 *            + up4(rows * h_l) + up4(rows * h_a) + up4(rows * h_v)                            their last hidden states
 *            + up4(rows * T * memsize) + up4(rows * T * gamma1) + up4(rows * T * gamma2)      cHat, the gamma partials
 *            + heads = 1: 2 * (up4(rows * zl) + up4(rows * za) + up4(rows * zv) + up4(rows * zy))   the chunk's means, logvars
 *              heads = 0: up4(N * zl) + up4(N * za) + up4(N * zv) + up4(N * zy)               the whole split's means
 *            + up4(rows * output_dim)                                                         the chunk's y_hat
 *            + up4(sum over m of ceil(T * rows / 64) * ceil(d_m / 64))                        the squared-error partials
 *            + heads = 0: up4(4 * ceil(N / (N <= 256 ? 8 : 32)))                              the MMD's partials
 *            + 12                                                                             five fp64 accumulators
 *            Beyond the row cap it grows with N by the whole-split means and the MMD's partials alone (heads = 0).
 * Determinism: the six values are bit-identical from run to run for a given (T, N, max_rows) and, heads = 0, a given gauss.
 * The recurrence launches run on one-row tiles while 6 * rows < 6 * CUs and on four-row tiles from there
 * (mfm_objective_mfn_tile_rows tells which; host only, -1 for bad arguments); the sums are fp64 in a fixed order per chunking.
 * Nothing outside the workspace and `out` is written.  T < 1, N < 1, a null pointer or max_rows < 0 return MFM_ERR_ARG before
 * anything touches the GPU.  MFM_ERR_UNSUPPORTED with the size in the error text, nothing enqueued: what mfm_encode_mfn refuses
 * (an h_dims entry or an encoder hidden size above 128, a windowsize other than 2, attention widths beyond the LDS, memsize or
 * gamma widths beyond the register-resident memory recurrence), what mfm_decode_factors refuses (a decoder with fy + f_m > 128,
 * more LDS than a CU has) and, heads = 0, a factor too wide for the MMD's LDS tiles (above about 300): run
 * mfm_plan_forward(train = 0) instead.  Stream-ordered, no host synchronisation, legal inside a stream capture. */
int64_t mfm_objective_mfn_workspace_floats(int32_t T, int64_t N, const int32_t* sizes /*host, 23*/, int64_t max_rows); /* host only; 0 for bad sizes */
int mfm_objective_mfn_tile_rows(int64_t N, int64_t max_rows);
int mfm_objective_mfn(int32_t T, int64_t N, const int32_t* sizes /*host, 23*/, const float* lambdas /*host, 4*/, const float* params,
                      const int64_t* offsets /*host, 100 or 86*/, const float* x, const void* y, const float* gauss /*[N, zl + za + zv + zy], or NULL*/,
                      float* workspace, float* out /*6*/, int64_t max_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * The zeroed-modality test protocol of MFM_KL_EF (csrc/zeros.hip; reference mfm_mosi.py:572-596, `predict` of
 * train_mfm_test_zeros): the split through the deterministic eval forward three times, each time with one modality's columns
 * taken as zero -- case 0: no l ([0, d_l)), 1: no a ([d_l, d_l + d_a)), 2: no v ([d_l + d_a, D)) -- in the pattern of the entries
 * above: fp32, dropout the identity, z = the mean heads, no MfmPlan, no training workspace, no zeroed copy of x and no x_hat in
 * memory.
 *   y_hat[c]  [N, output_dim]: y_hat of case c
 *   gen[c]    mean over T * N * d_c of (x_c_hat of case c - the REAL x_c)^2: F.mse_loss as the reference prints it, unweighted
 *   disc[c]   mean L1 (loss_kind 0) / cross entropy (1) of y_hat[c], as mfm_predict_klef defines it
 * Only what these depend on runs (mfm_model.py:619-660): the ef encoder on the three zeroed inputs, encoder_c on zeros -- the
 * same row z_c^0 for every sample --, decoder_c of case c, the classifier.  The encoders of the present modalities reach none of
 * the results and do not run.  Per row chunk: ONE grouped fp32 GEMM of the ef encoder's input projection split by modality
 * (P_m = x_m W_ih[:, columns of m]^T: every column of x meets W_ih once for the three cases); one pass that forms the gates of
 * case c as the sum of the P_m, m != c, plus b_ih + b_hh; ONE launch of (ef encoder, case, row tile) workgroups (recurrence, fc1,
 * last_to_zy_fc1 -> zy_c) which in the first chunk carries three more one-row workgroups for the z_c^0; the recurrence launch of
 * mfm_decode_factors with decoder c on (z_c^0, zy_c), every decoder's workgroups also the classifier -> y_hat[c]; the fused fc1 /
 * squared-error launch of mfm_objective_klef against the real x; one single-workgroup launch that adds the chunk's partials and
 * label-loss terms in a fixed order into fp64 accumulators and, behind the last chunk, divides by the counts of the WHOLE split.
 * No float atomics: the results are bit-identical from run to run for a given (T, N, max_rows).
 *   sizes    host, 13: as mfm_objective_klef
 *   offsets  host, 78 element offsets into the flat fp32 parameter buffer `params`: as mfm_objective_klef (the logvar heads'
 *            are not read)
 *   x        [T, N, D] time-major and contiguous, 4-byte aligned (any contiguous view); it is read only, all of it
 *   y        NULL, or the labels: float [N, output_dim] (loss_kind 0) / int64 [N] (loss_kind 1)
 *   y_hat    out, [3, N, output_dim]; gen: out, 3 device floats; disc: out, 3 device floats -- NULL exactly when y is
 *   max_rows row cap: chunks of at most max_rows rows (0: one chunk) that share the workspace; every mean is over the whole
 *            split whatever the chunking
 *   workspace mfm_predict_zeros_klef_workspace_floats(T, N, sizes, max_rows) floats, 16-byte aligned, contents arbitrary; with
 *            rows = min(N, max_rows): the larger of 6 * rows * T * 4 * round_up(zl + za + zv, 16) (three partial projections,
 *            three gate sets) and the workspace of mfm_decode_factors (the stored h takes their place), the constant gates and
 *            rows of the zeroed encoders, zy of the three cases, one partial per workgroup of the squared-error launch, and the
 *            accumulators -- it does not grow with N beyond the row cap
 * Nothing outside the workspace, y_hat, gen and disc is written.  T < 1, N < 1, a null pointer or max_rows < 0 return MFM_ERR_ARG
 * before anything touches the GPU.  Any N >= 1 (< 2^24), T >= 1.  Sizes the on-chip recurrence does not cover (a hidden size > 128,
 * or more LDS than a CU has) return MFM_ERR_UNSUPPORTED with the size in the error text and enqueue nothing: run
 * mfm_plan_forward(train = 0) on zeroed copies instead.  Stream-ordered, no host synchronisation, legal inside a stream capture. */
int64_t mfm_predict_zeros_klef_workspace_floats(int32_t T, int64_t N, const int32_t* sizes /*host, 13*/, int64_t max_rows); /* host only; 0 for bad sizes */
int mfm_predict_zeros_klef(int32_t T, int64_t N, const int32_t* sizes /*host, 13*/, const float* params, const int64_t* offsets /*host, 78*/,
                           const float* x, const void* y /*or NULL*/, float* workspace, float* y_hat /*[3, N, output_dim]*/,
                           float* gen /*3*/, float* disc /*3, or NULL*/, int64_t max_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * mfm_predict_zeros_mfn (csrc/zeros_mfn.hip): the same protocol, with the same results y_hat[c], gen[c], disc[c] and under the
 * same contract, for MFM_KL and MFM, whose label factor comes from the Memory Fusion Network (mfm_model.py:140-199, :723-743).
 * Only what the results depend on runs: the MFN's three LSTMs on the real columns of x ONCE for the three cases (they are
 * independent of each other); the MFN LSTM and the encoder of a zeroed modality on the all-zero row, one row of work each;
 * decoder c of case c; the classifier.  The present modalities' own encoders reach none of the results and do not run; no
 * log-variance head, no KLD and no MMD is computed.  heads = 1 (MFM_KL): z_c^0 = last_to_z{c}_fc1(encoder_c(0)); heads = 0
 * (MFM): z_c^0 = encoder_c(0), its fc1 output.  Per row chunk of n rows: ONE grouped fp32 GEMM for the three input projections;
 * ONE launch of (MFN LSTM, row tile) workgroups that store the cell states and the last hidden state, which in the first chunk
 * carries six more one-row workgroups on the constant gates b_ih + b_hh (a small launch fills them in front) -- the three MFN
 * LSTMs on zero input (a one-row cell-state record and last h) and the three encoders on zero input (fc1, the mean head with
 * heads: z_c^0); the attention chain of mfm_encode_mfn over the 3 * T * n triples (t, case, row), cStar gathered with modality
 * c's columns from the one-row record; its memory recurrence per (case, row) ending with last_to_zy_fc1 on [h_l | h_a | h_v |
 * mem], h_c the zero row's -> zy_c; then the launches of mfm_predict_zeros_klef from the decoders on: decoder c on (zy_c,
 * z_c^0) with the classifier -> y_hat[c], the fused fc1 / squared-error launch against the real x, and the fp64 finish.
 *   sizes    host, 23: the 17 of mfm_encode_mfn (d_l, d_a, d_v; zl, za, zv; zy; h_l, h_a, h_v; memsize; windowsize; the hidden
 *            widths of att1, att2, gamma1, gamma2; heads), then fl, fa, fv, fy, output_dim, loss_kind (0 = L1, 1 = cross entropy)
 *   offsets  host, element offsets into the flat fp32 parameter buffer `params`: the 62 (heads = 1) or 48 (heads = 0) of
 *            mfm_encode_mfn in its order (the logvar heads' are not read), then the 38 of mfm_decode_factors: 100 or 86
 *   x, y, y_hat, gen, disc, max_rows   as mfm_predict_zeros_klef
 *   workspace mfm_predict_zeros_mfn_workspace_floats(T, N, sizes, max_rows) floats, 16-byte aligned, contents arbitrary.  With
 *            rows = min(N, max_rows), Hp(h) = round_up(h, 16), up4(v) = round_up(v, 4):
 *              max(rows * T * 4 * (Hp(h_l) + Hp(h_a) + Hp(h_v)),                              the x-projections, and in their
 *                  rows * T * (Hp(fy + fl) + Hp(fy + fa) + Hp(fy + fv)))                      place the decoders' stored h
 *            + rows * T * (Hp(h_l) + Hp(h_a) + Hp(h_v))                                       the MFN LSTMs' cell states
 *            + up4(rows * h_l) + up4(rows * h_a) + up4(rows * h_v)                            their last hidden states
 *            + up4(3 * rows * T * memsize) + up4(3 * rows * T * gamma1) + up4(3 * rows * T * gamma2)    cHat, the gamma partials
 *            + T * 4 * (Hp(h_l) + Hp(h_a) + Hp(h_v) + Hp(zl) + Hp(za) + Hp(zv))               the six constant gate sets
 *            + T * (Hp(h_l) + Hp(h_a) + Hp(h_v)) + up4(h_l) + up4(h_a) + up4(h_v)             the one-row records and last h
 *            + up4(rows * zl) + up4(rows * za) + up4(rows * zv)                               z_c^0, one row per chunk row
 *            + up4(3 * rows * zy)                                                             zy of the three cases
 *            + up4(sum over m of ceil(T * rows / 64) * ceil(d_m / 64))                        the squared-error partials
 *            + 12                                                                             six fp64 accumulators
 * Determinism: no float atomics; bit-identical from run to run for a given (T, N, max_rows).  The recurrence launch and the
 * decoders' run on one-row tiles while 3 * rows < 6 * CUs and on four-row tiles from there (mfm_predict_zeros_mfn_tile_rows
 * tells which; host only, -1 for bad arguments); the attention chain takes 16 or 32 triples per workgroup, a triple's
 * arithmetic the same in both.  For a fixed tile-row form y_hat is bit-identical for every row chunking; gen and disc are fp64
 * sums in a fixed order per chunking, over the counts of the WHOLE split.
 * Nothing outside the workspace, y_hat, gen and disc is written.  T < 1, N < 1, a null pointer or max_rows < 0 return MFM_ERR_ARG
 * before anything touches the GPU.  MFM_ERR_UNSUPPORTED with the size in the error text, nothing enqueued: what mfm_encode_mfn
 * refuses (an h_dims entry or an encoder hidden size above 128, a windowsize other than 2, attention widths beyond the LDS,
 * memsize or gamma widths beyond the register-resident memory recurrence) and what mfm_decode_factors refuses (a decoder with
 * fy + f_m > 128, more LDS than a CU has): run mfm_plan_forward(train = 0) on zeroed copies instead.  Stream-ordered, no host
 * synchronisation, legal inside a stream capture. */
int64_t mfm_predict_zeros_mfn_workspace_floats(int32_t T, int64_t N, const int32_t* sizes /*host, 23*/, int64_t max_rows); /* host only; 0 for bad sizes */
int mfm_predict_zeros_mfn_tile_rows(int64_t N, int64_t max_rows);
int mfm_predict_zeros_mfn(int32_t T, int64_t N, const int32_t* sizes /*host, 23*/, const float* params, const int64_t* offsets /*host, 100 or 86*/,
                          const float* x, const void* y /*or NULL*/, float* workspace, float* y_hat /*[3, N, output_dim]*/,
                          float* gen /*3*/, float* disc /*3, or NULL*/, int64_t max_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * mfm_predict_mfn (csrc/predict_mfn.hip): the prediction-only path of MFM_KL and MFM -- what mfm_predict_klef is for MFM_KL_EF,
 * under its contract, for the classes whose label factor comes from the Memory Fusion Network (mfm_model.py:140-199, :723-743):
 *   zy = last_to_zy_fc1([h_l,T | h_a,T | h_v,T | mem_T]) of the MFN as mfm_encode_mfn defines it (the mean; nothing is sampled),
 *   fy = relu(zy_to_fy_fc2(relu(zy_to_fy_fc1(zy)))), y_hat = fy_to_y_fc2(relu(fy_to_y_fc1(fy))),
 *   *loss = mean |y_hat - y| over N * output_dim (loss_kind 0) / mean cross entropy over N (1), as mfm_predict_klef defines it.
 * Only what these depend on runs: the three modality encoders and their heads, every log-variance head, KLD / MMD, the
 * modalities' z -> f MLPs, the decoders and their fc1 do not, and their parameters are not read.  Per row chunk of n rows, on the
 * one stream given: ONE grouped fp32 GEMM for the three input projections; ONE launch of (MFN LSTM, row tile) workgroups that
 * store the cell states and the last hidden state; the attention chain of mfm_encode_mfn over the T * n pairs; its memory
 * recurrence per row, which keeps zy in LDS and goes on, in the same workgroup, with the four small layers -- it writes the row
 * of y_hat and, with labels, the row's loss contribution.  The workgroup that draws the LAST arrival ticket of a chunk adds the
 * chunk's contributions in a fixed order in fp64 onto the running sum of the chunks before it and, behind the last chunk,
 * divides by the counts of the WHOLE split; it puts the ticket word back to 0.  Nobody waits or spins, no float atomics touch
 * the result.
 *   sizes    host, 23: as mfm_predict_zeros_mfn.  zl, za, zv and fl, fa, fv must be positive and are otherwise unused; heads
 *            (entry 16) must be 0 or 1 and is otherwise unused: the label path is the same for MFM_KL and MFM
 *   offsets  host, 38 element offsets into the flat fp32 parameter buffer `params`: per MFN LSTM l, a, v weight_ih, weight_hh,
 *            bias_ih, bias_hh (12); weight and bias of att1_fc1, att1_fc2, att2_fc1, att2_fc2, gamma1_fc1, gamma1_fc2, gamma2_fc1,
 *            gamma2_fc2 (16); of last_to_zy_fc1 (2); of zy_to_fy_fc1, zy_to_fy_fc2, fy_to_y_fc1, fy_to_y_fc2 (8) (torch layouts; the
 *            LSTM weights 16-byte aligned)
 *   x        [T, N, D] time-major and contiguous, D = d_l + d_a + d_v, 4-byte aligned: any contiguous view; read only
 *   y        NULL, or the labels: float [N, output_dim] (loss_kind 0) / int64 [N] (loss_kind 1, class indices)
 *   y_hat    out, [N, output_dim]; loss: out, one device float -- NULL exactly when y is (then no loss is computed or written)
 *   max_rows row cap: chunks of at most max_rows rows (0: one chunk) that share the workspace; the loss is the mean over all N
 *            rows whatever the chunking
 *   workspace mfm_predict_mfn_workspace_floats(T, N, sizes, max_rows) floats, 16-byte aligned, contents arbitrary.  With
 *            rows = min(N, max_rows), Hp(h) = round_up(h, 16), up4(v) = round_up(v, 4), in this order:
 *              rows * T * 4 * (Hp(h_l) + Hp(h_a) + Hp(h_v))                                   the x-projections
 *            + rows * T * (Hp(h_l) + Hp(h_a) + Hp(h_v))                                       the MFN LSTMs' cell states
 *            + up4(rows * h_l) + up4(rows * h_a) + up4(rows * h_v)                            their last hidden states
 *            + up4(rows * T * memsize) + up4(rows * T * gamma1) + up4(rows * T * gamma2)      cHat, the gamma partials
 *            + up4(rows)                                                                      one loss contribution per chunk row
 *            + 4                                                                              the fp64 running sum, the ticket word, a pad
 *            It does not grow with N beyond the row cap.  With labels the call clears the ticket word itself (a memset on the
 *            stream) and leaves it at 0: it is the third of the last four floats.
 * Determinism: bit-identical from run to run for a given (T, N, max_rows).  The recurrence launch runs on one-row tiles while
 * 3 * rows < 6 * CUs and on four-row tiles from there (mfm_predict_mfn_tile_rows tells which; host only, -1 for bad arguments);
 * the attention chain takes 16 or 32 pairs per workgroup, a pair's arithmetic the same in both.  For a fixed tile-row form y_hat
 * is bit-identical for every row chunking; the loss is an fp64 sum in a fixed order per chunking.
 * Nothing outside the workspace, y_hat and *loss is written; rows beyond a chunk are neither read nor written.  T < 1, N < 1, a
 * null pointer, y without loss or loss without y, or max_rows < 0 return MFM_ERR_ARG before anything touches the GPU.
 * MFM_ERR_UNSUPPORTED with the size in the error text, nothing enqueued: an h_dims entry above 128, a windowsize other than 2,
 * attention widths beyond the LDS, memsize or gamma widths beyond the register-resident memory recurrence, a label head's input
 * and tail activations (the widest of zy, fy, output_dim, twice) beyond the LDS: run mfm_plan_forward(train = 0) instead.
 * Stream-ordered, no host synchronisation, no allocation, legal inside a stream capture (no forked branches). */
int64_t mfm_predict_mfn_workspace_floats(int32_t T, int64_t N, const int32_t* sizes /*host, 23*/, int64_t max_rows); /* host only; 0 for bad sizes */
int mfm_predict_mfn_tile_rows(int64_t N, int64_t max_rows);
int mfm_predict_mfn(int32_t T, int64_t N, const int32_t* sizes /*host, 23*/, const float* params, const int64_t* offsets /*host, 38*/,
                    const float* x, const void* y /*or NULL*/, float* workspace, float* y_hat /*[N, output_dim]*/,
                    float* loss /*or NULL*/, int64_t max_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * The gradient-based interpretation of the factorized model (csrc/influence.hip): how strongly the factors drive the generation
 * of each modality at each time step.  For decoder m = l, a, v with embedding e = [fy | f_m] of width h = fy + f_m
 * (mfm_model.py:644-656, decoderLSTM :64-91), from the deterministic eval computation (dropout the identity),
 *   out[0][m][t][n] = sum_{i < d_m} sum_{j < fy}       (d x_m_hat[t][n][i] / d e[n][j])^2      ("fy")
 *   out[1][m][t][n] = sum_{i < d_m} sum_{fy <= j < h}  (d x_m_hat[t][n][i] / d e[n][j])^2      ("fm")
 * The derivative is with respect to the factors f, behind the z -> f MLPs.  Forward mode: the h tangent columns of a row are
 * carried along the decoder's recurrence, J^a = (W_ih + W_hh) J^h (step 0: W_ih itself) and J^x = W_fc1 J^h on
 * v_mfma_f32_16x16x4_f32, the gate-derivative scalings on the VALU, h, c, J^h and J^c in LDS; fp32 throughout.  One small launch
 * per call packs the decoders' weights into the workspace (gate-interleaved rows, padded to the MFMA tile with exact zeros);
 * then per row chunk ONE launch whose workgroups are (decoder, row tile): fy and f_m of the tile's rows on the code path of
 * mfm_decode_factors (bit-identical embedding), the T steps, and per step the sums of squares reduced inside the workgroup in
 * a fixed order.  Every out element is stored once by one workgroup; no Jacobian and no x_hat leaves the chip; no atomics:
 * results are bit-identical from run to run and for every max_rows.
 *   sizes, offsets, z   exactly the arguments of mfm_decode_factors (the classifier's offsets are not read)
 *   out      [2, 3, T, N] device floats (4-byte aligned): block (fy, fm), decoder (l, a, v)
 *   max_rows row cap: chunks of at most max_rows rows (0: one chunk)
 *   workspace mfm_influence_factors_workspace_floats(T, N, sizes, max_rows) floats, 16-byte aligned, contents arbitrary: per
 *            decoder, with Hp = round_up(fy + f_m, 16), 8 Hp^2 + 4 Hp + round_up(d_m, 16) Hp for the packed weights -- it does
 *            not depend on T, N or max_rows
 * Nothing outside the workspace and `out` is written.  T < 1, N < 1, a null pointer or max_rows < 0 return MFM_ERR_ARG before
 * anything touches the GPU.  A decoder with fy + f_m > 128, or more LDS than a CU has, returns MFM_ERR_UNSUPPORTED with the
 * size in the error text and enqueues nothing.  Stream-ordered, no host synchronisation, legal inside a stream capture. */
int64_t mfm_influence_factors_workspace_floats(int32_t T, int64_t N, const int32_t* sizes /*host, 12*/, int64_t max_rows); /* host only; 0 for bad sizes */
int mfm_influence_factors(int32_t T, int64_t N, const int32_t* sizes /*host, 12*/, const float* params, const int64_t* offsets /*host, 38*/,
                          const float* const* z /*host, 4*/, float* workspace, float* out /*[2, 3, T, N]*/, int64_t max_rows,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * Surrogate inference of MFM_missing (csrc/impute.hip; reference mfm_model.py:766-885, evaluated in mfm_mosi.py:572-596 and
 * :1023-1062): a missing modality m and the label from the other two modalities, in the pattern of the entries above -- fp32,
 * dropout the identity, no MfmPlan, no training workspace.  For every case m asked for
 *   z_m' = encoder_<pair>_to_<m>(pair), zy' = encoder_<pair>_to_y(pair), pair = cat of the two observed modalities' columns of x
 *   fy = relu(zy_to_fy_fc2(relu(zy_to_fy_fc1(zy')))), f_m likewise from z_m' through z<m>_to_f<m>
 *   x_hat_m = decoder_m(cat([fy, f_m]), T),  y_hat_m = fy_to_y_fc2(relu(fy_to_y_fc1(fy)))
 * which are decoded_no<m>[index of m] and decoded_no<m>[3] of MFM_missing.forward.  THE COLUMNS OF m ARE NEVER READ (case l:
 * [0, d_l), case a: [d_l, d_l + d_a), case v: [d_l + d_a, D)): they may hold anything.  Per row chunk: a copy launch gathers the
 * observed pair of every case into the workspace as a zero-padded matrix of its own (the GEMM masks the 16-byte fetches that
 * pass a row's K range by multiplication: on a column range of x they would meet the missing modality's columns, and a NaN
 * there would survive the mask); the input projections of the cases' surrogate encoders as one grouped GEMM on those copies;
 * ONE launch of (encoder, row tile) workgroups (recurrence + fc1 -> the z rows, into the workspace); ONE launch of (case, row
 * tile) workgroups (the z -> f MLPs, the classifier, the decoder recurrence storing h_t); the decoders' fc1 as one grouped
 * GEMM into x_hat_m.  No workgroup waits for another.
 *   sizes    host, 12: zl, za, zv, zy, fl, fa, fv, fy, d_l, d_a, d_v, output_dim; x [T, N, D] time-major and contiguous (4-byte aligned: any contiguous view)
 *   cases    bit 0: l missing, bit 1: a, bit 2: v; one bit, or all three (7: the three cases share the launches)
 *   params   host array of 74 DEVICE pointers to the module's own tensors (torch layouts, contiguous fp32; the LSTM weights
 *            16-byte aligned, the rest 4), per case m = l, a, v at 22 * m: the encoder -> z_m (av_to_l / lv_to_a / la_to_v): lstm
 *            weight_ih, weight_hh, bias_ih, bias_hh, fc1 weight, bias; the encoder -> zy (av_to_y / lv_to_y / la_to_y) alike;
 *            z<m>_to_f<m> fc1 weight, bias, fc2 weight, bias; decoder_m lstm weight_ih, weight_hh, bias_ih, bias_hh, fc1
 *            weight, bias.  Then at 66: weight and bias of zy_to_fy_fc1, zy_to_fy_fc2, fy_to_y_fc1, fy_to_y_fc2.  The 22 of a case
 *            not asked for are not read and may be null
 *   out      host array of 6 device pointers: x_hat_l [T, N, d_l], y_hat_l [N, output_dim], x_hat_a, y_hat_a, x_hat_v, y_hat_v;
 *            those of a case not asked for are not read
 *   max_rows row cap: chunks of at most max_rows rows (0: one chunk) that share the workspace
 *   workspace mfm_impute_missing_workspace_floats(T, N, sizes, cases, max_rows) floats, 16-byte aligned, contents arbitrary; with
 *            rows = min(N, max_rows), per case: rows * T * 4 * (round_up(z_m, 16) + round_up(zy, 16)) for the x-projections,
 *            round_up(rows * z_m, 4) + round_up(rows * zy, 4) for the z rows, rows * T * round_up(fy + f_m, 16) for the stored h,
 *            and rows * T * (round_up(k_m, 4) + 4) for the gathered pair, k_m = D - d_m
 * mfm_impute_missing_tile_rows: host only; rows per workgroup the two recurrence launches of such a call use (tile_rows[0] the
 * encoders', [1] the decoders': 1 below six workgroups per CU over the launch, else 4).  Results are bit-identical from call to
 * call and across row caps that keep the tile rows.
 * Nothing outside the workspace and the outputs is written.  Any N >= 1 (< 2^24), T >= 1.  Sizes the on-chip recurrence does not
 * cover (a hidden size > 128, or more LDS than a CU has) return MFM_ERR_UNSUPPORTED with the size in the error text and enqueue
 * nothing: compose the granular entries instead.  Stream-ordered, no host synchronisation, legal inside a stream capture. */
int64_t mfm_impute_missing_workspace_floats(int32_t T, int64_t N, const int32_t* sizes /*host, 12*/, int32_t cases,
                                            int64_t max_rows); /* host only; 0 for bad sizes */
int mfm_impute_missing_tile_rows(int64_t N, int32_t cases, int64_t max_rows, int32_t* tile_rows /*host, 2*/);
int mfm_impute_missing(int32_t T, int64_t N, const int32_t* sizes /*host, 12*/, int32_t cases, const float* const* params /*host, 74*/,
                       const float* x, float* workspace, float* const* out /*host, 6*/, int64_t max_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * The missing-modality test protocol (csrc/missing.hip; the `predict` / `score` blocks of the reference's train_mfm_missing,
 * seq2seq and basic_missing loops, reference mfm_model.py:766-1017): per missing case m the error of the rebuilt modality, the
 * label prediction and its label loss, for the three classes of the missing-modality family, in the pattern of
 * mfm_impute_missing and mfm_predict_zeros_klef -- fp32, dropout the identity, no MfmPlan, no x_hat written.
 *   family 0, MFM_missing    y_hat_m = decoded_no<m>[3] and x_hat_m = decoded_no<m>[index of m] as mfm_impute_missing computes them;
 *                            gen_m = mean((x_hat_m - x_m)^2), disc_m = the mean label loss of y_hat_m
 *   family 1, seq2seq        x_hat_m = decoder_m(relu(z<m>_to_f<m>_fc2(relu(z<m>_to_f<m>_fc1(encoder_<pair>_to_<m>(pair))))), T),
 *                            gen_m = mean((x_hat_m - x_m)^2); no label path: y, y_hat and disc are not looked at
 *   family 2, basic_missing  y_hat_m = zy_no<m>_to_y_fc2(relu(zy_no<m>_to_y_fc1(encoder_<pair>_to_y(pair)))), disc_m; no decoder:
 *                            gen is not looked at
 * pair = cat of the two observed modalities' columns of x.  THE COLUMNS OF m REACH THE SQUARED ERROR ALONE, as its target: no
 * encoder, y_hat_m or disc_m depends on them, and family 2 never reads them.  Per row chunk: the gather of the observed pairs
 * and the grouped x-projection GEMM of mfm_impute_missing; the encoder recurrences (families 0, 1: those of mfm_impute_missing;
 * family 2: ONE launch of (case, row tile) workgroups that go on to the encoder's fc1 and the case's head and write y_hat); the
 * decoder recurrences storing h_t (family 0: the launch of mfm_impute_missing; family 1: ONE launch of (case, row tile)
 * workgroups without the fy half); the decoders' fc1 fused with the squared error, one partial per workgroup; one workgroup that
 * adds the partials and the label loss in fp64 in a fixed order -- no float atomics.
 *   sizes, cases  as mfm_impute_missing; a size the family does not have (family 1: zy, fy, output_dim; family 2: z_m, f_m) may be
 *            any positive value
 *   loss_kind 0: L1 against float labels y [N, output_dim]; 1: cross entropy against int64 class indices y [N] (8-byte aligned)
 *   params   host array of 74 DEVICE pointers laid out as mfm_impute_missing's.  Family 0: all of them.  Family 1, per case at
 *            22 * m: 0-5 the encoder -> z_m, 12-15 z<m>_to_f<m> fc1 weight, bias, fc2 weight, bias, 16-21 decoder_m (h = f_m).
 *            Family 2, per case at 22 * m: 6-11 the encoder -> zy (av_to_y / lv_to_y / la_to_y), 12-15 zy_no<m>_to_y fc1 weight,
 *            bias, fc2 weight, bias.  Slots a family does not have, and the 22 of a case not asked for, are not read and may be null
 *   y        labels of the whole split, or null: no label loss (then disc must be null too)
 *   y_hat    cases = 7: [3, N, output_dim] in the order l, a, v; one case: [N, output_dim]
 *   gen, disc  3 floats each whatever the cases, case m's at index m, written behind the last chunk; with one case the other two
 *            entries are overwritten with values that mean nothing
 *   workspace mfm_predict_missing_workspace_floats(T, N, sizes, family, cases, with_labels, max_rows) floats, 16-byte aligned,
 *            contents arbitrary: per case what mfm_impute_missing keeps of it for the family's launches, then one float per
 *            squared-error workgroup of a chunk, six fp64 accumulators and 4 floats (for family 0 never less than
 *            mfm_impute_missing_workspace_floats)
 * mfm_predict_missing_tile_rows: host only; rows per workgroup of the encoders' launch (tile_rows[0]) and of the decoders'
 * ([1]; 0 for family 2, which has none): 1 below six workgroups per CU over the launch, else 4.  The encoders' launch counts two
 * LSTMs per case for family 0, one for families 1 and 2.  Results are bit-identical from call to call; y_hat also across row
 * caps that keep the tile rows (gen and disc then differ in the grouping of the fp64 sums alone).
 * Nothing outside the workspace and the three outputs is written.  Any N >= 1 (< 2^24), T >= 1.  Sizes the on-chip recurrence does
 * not cover (a hidden size > 128, or more LDS than a CU has) return MFM_ERR_UNSUPPORTED with the size in the error text and
 * enqueue nothing: compose the granular entries instead.  Bad arguments return MFM_ERR_ARG and enqueue nothing.  Stream-ordered,
 * no host synchronisation, legal inside a stream capture. */
int64_t mfm_predict_missing_workspace_floats(int32_t T, int64_t N, const int32_t* sizes /*host, 12*/, int32_t family, int32_t cases,
                                             int32_t with_labels, int64_t max_rows); /* host only; 0 for bad sizes */
int mfm_predict_missing_tile_rows(int64_t N, int32_t family, int32_t cases, int64_t max_rows, int32_t* tile_rows /*host, 2*/);
int mfm_predict_missing(int32_t T, int64_t N, const int32_t* sizes /*host, 12*/, int32_t family, int32_t cases, int32_t loss_kind,
                        const float* const* params /*host, 74*/, const float* x, const void* y /*null: no label loss*/,
                        float* workspace, float* y_hat, float* gen, float* disc, int64_t max_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * Prediction of the ablations M_B and M_D (csrc/ablation.hip; the `evaluate` / `predict` blocks of the reference's
 * train_mfm_ablation, reference mfm_mosi.py:640-767, mfm_model.py:317-343 and :445-467): the label prediction, its label loss
 * and (M_B) the three reconstruction errors, in the pattern of mfm_predict_missing -- fp32, dropout the identity, no MfmPlan, no
 * training workspace, no x_hat written.  Both classes run three independent own-modality encoders that meet at the label head:
 *   family 0, M_B   z_m = encoder_m(x_m), f_m = relu(z<m>_to_f<m>_fc2(relu(z<m>_to_f<m>_fc1(z_m)))) for m in l, a, v;
 *                   y_hat = fy_to_y_fc2(relu(fy_to_y_fc1([f_l | f_a | f_v]))); gen_m = mean((decoder_m(f_m, T) - x_m)^2)
 *   family 1, M_D   the same three encoders and z -> f MLPs; y_hat = fs_to_y([f_l | f_a | f_v]); no decoders: gen must be null and
 *                   with_gen 0
 * Per row chunk: the three input projections as one grouped GEMM on the column ranges of x; ONE launch of (encoder m, row tile)
 * workgroups, each of which runs its recurrence, the encoder's fc1 and the z -> f MLP on chip, stores its f_m rows into the
 * workspace and draws an arrival ticket for its row tile -- the workgroup that draws the last of a tile's three tickets reads
 * the tile's f rows, runs the label head, writes the tile's rows of y_hat and, with labels, one loss contribution per row; the
 * last tile of a chunk to finish adds the chunk's contributions in fp64 in a fixed order.  No workgroup waits for another, every
 * ticket word is 0 again when the call ends (a captured graph can be replayed), z_m is never written.  With gen: ONE launch of
 * (decoder m, row tile) workgroups storing h_t (h = f_m), the decoders' fc1 fused with the squared error, one partial per
 * workgroup, and one workgroup that adds the partials in fp64 in a fixed order -- no float atomics anywhere.
 *   sizes    host, 12, the layout of mfm_predict_missing: zl, za, zv, zy, fl, fa, fv, fy, d_l, d_a, d_v, output_dim; zy is unused, fy
 *            is the classifier's hidden width (M_B; unused for M_D); an unused entry may be any positive value.  x [T, N, D]
 *            time-major and contiguous (4-byte aligned: any contiguous view)
 *   loss_kind 0: L1 against float labels y [N, output_dim]; 1: cross entropy against int64 class indices y [N] (8-byte aligned)
 *   with_gen 1: gen is computed (family 0 alone) and must not be null; 0: gen must be null, no decoder runs
 *   params   host array of 52 DEVICE pointers to the module's own tensors (torch layouts, contiguous fp32; the LSTM weights
 *            16-byte aligned, the rest 4), per modality m = l, a, v at 16 * m: 0-5 encoder_m: lstm weight_ih, weight_hh, bias_ih,
 *            bias_hh, fc1 weight, bias; 6-9 z<m>_to_f<m> fc1 weight, bias, fc2 weight, bias; 10-15 decoder_m alike the encoder
 *            (h = f_m) -- not read, and may be null, when with_gen is 0 or family is 1.  Then at 48, M_B: fy_to_y_fc1 weight, bias,
 *            fy_to_y_fc2 weight, bias; M_D: fs_to_y weight, bias, and 50-51 are not read
 *   y        labels of the whole split, or null: no label loss (then disc must be null too)
 *   y_hat    [N, output_dim];  gen  3 floats in the order l, a, v;  disc  1 float, the mean over the WHOLE split whatever the
 *            chunking; gen and disc are written behind the last chunk
 *   max_rows row cap: chunks of at most max_rows rows (0: one chunk) that share the workspace
 *   workspace mfm_predict_ablation_workspace_floats(T, N, sizes, family, with_gen, with_labels, max_rows) floats, 16-byte aligned,
 *            contents arbitrary; with rows = min(N, max_rows), in this order: rows * T * 4 * (round_up(zl, 16) + round_up(za, 16)
 *            + round_up(zv, 16)) for the x-projections; round_up(rows * (fl + fa + fv), 4) for the f rows; with gen rows * T *
 *            (round_up(fl, 16) + round_up(fa, 16) + round_up(fv, 16)) for the stored h, one float per squared-error workgroup of
 *            a chunk (the sum over m of ceil(T * rows / 64) * ceil(d_m / 64), rounded up to 4) and 12 for six fp64 accumulators;
 *            with labels round_up(rows, 4) loss contributions; round_up(rows, 4) ticket words; and 4 floats for the fp64 running
 *            sum of the loss and the chunk's ticket word
 * mfm_predict_ablation_tile_rows: host only; rows per workgroup of the encoders' launch (tile_rows[0]) and of the decoders'
 * ([1]; 0 without gen): 1 below six workgroups per CU over the launch, else 4; both launches count three LSTMs.  Results are
 * bit-identical from call to call; y_hat also across row caps that keep the tile rows (gen and disc then differ in the grouping
 * of the fp64 sums alone); y_hat and disc have the same bits with and without gen.
 * Nothing outside the workspace and the three outputs is written.  Any N >= 1 (< 2^24), T >= 1.  Sizes the on-chip recurrence does
 * not cover (a z_m > 128, an f_m > 128 with gen, more LDS than a CU has, or a label head whose input row fl + fa + fv and
 * activations do not fit the LDS) return MFM_ERR_UNSUPPORTED with the size in the error text and enqueue nothing: compose the
 * granular entries instead.  Bad arguments (T or N < 1, N >= 2^24, a null pointer, y without disc or disc without y, gen without
 * with_gen or with_gen without gen, either of them for family 1, max_rows < 0, a family outside {0, 1}) return MFM_ERR_ARG and
 * enqueue nothing.  Stream-ordered, no host synchronisation, no allocation; legal inside a stream capture on the one given
 * stream (no forked branches). */
int64_t mfm_predict_ablation_workspace_floats(int32_t T, int64_t N, const int32_t* sizes /*host, 12*/, int32_t family, int32_t with_gen,
                                              int32_t with_labels, int64_t max_rows); /* host only; 0 for bad sizes */
int mfm_predict_ablation_tile_rows(int64_t N, int32_t family, int32_t with_gen, int64_t max_rows, int32_t* tile_rows /*host, 2*/);
int mfm_predict_ablation(int32_t T, int64_t N, const int32_t* sizes /*host, 12*/, int32_t family, int32_t loss_kind, int32_t with_gen,
                         const float* const* params /*host, 52*/, const float* x, const void* y /*null: no label loss*/,
                         float* workspace, float* y_hat, float* gen /*3, or null*/, float* disc /*1, or null*/, int64_t max_rows,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * One training step of the ablation M_D without the optimizer (csrc/train_ablation.hip; the `train` block of the reference's
 * train_mfm_ablation, reference mfm_mosi.py:640-767, for mfm_model.py:389-467): the mean label loss of the split and its gradient
 * with respect to all 32 parameter tensors, fp32 throughout, no MfmPlan.  The class is purely discriminative:
 *   z_m = encoder_m.fc1(h_T,m), f_m = relu(z<m>_to_f<m>_fc2(drop_m(relu(z<m>_to_f<m>_fc1(z_m))))) for m in l, a, v;
 *   y_hat = fs_to_y([f_l | f_a | f_v]); loss = L1 or cross entropy of y_hat, the mean over all N rows
 * Per row chunk, in this order on the one given stream: (1) the three input projections x_m W_ih^T + b_ih + b_hh as one grouped
 * fp32 GEMM into gate records; (2) one forward recurrence launch for the three encoders, the BPTT record (gates, hs, cs) kept;
 * (3) one launch of the head kernel over row tiles: a workgroup goes from h_T through the ten linears to y_hat (stored) and the
 * row's loss contribution and straight back to d h_T,m (stored), and stores ONE partial of the ten weight / bias gradients; the
 * workgroup that draws the launch's last arrival ticket adds the partials tile by tile in a fixed order and stores or adds the
 * gradients, adds the loss contributions in fp64 in a fixed order onto the running sum, writes the mean behind the last chunk and
 * puts the ticket word back to 0 -- no float atomic touches a result, no workgroup waits for another; (4) one BPTT launch for
 * the three encoders with dh_ext = the stored d h_T,m; (5) one grouped GEMM, unsplit along K, for dW_ih, dW_hh (skipped when
 * T == 1: nothing feeds W_hh, and a stored gradient is cleared with a memset node instead) and both bias gradients of the three
 * encoders.  dx is not computed.  A chunk of a longer split (max_rows < N) is first copied out of x as one [T n, D] matrix (a
 * 2-D copy node).  Loss, y_hat and gradients are bit-identical from call to call for a given (T, N, max_rows).
 *   sizes    host, 12, the layout of mfm_predict_ablation: zl, za, zv, zy, fl, fa, fv, fy, d_l, d_a, d_v, output_dim; zy and fy are
 *            unused and may be any positive value.  x [T, N, D] time-major and contiguous (4-byte aligned: any contiguous view)
 *   loss_kind 0: L1 against float labels y [N, output_dim]; 1: cross entropy against int64 class indices y [N] (8-byte aligned).
 *            The indices must lie in [0, output_dim): the labels are device data and are not checked; an index outside the
 *            range is clamped to the nearest class (so that nothing outside the row is read) and loss and gradients are then
 *            those of that class, without an error
 *   train, p_drop, seed, call, tick  dropout of the three z -> f MLPs: with train != 0 and p_drop[m] > 0 (host, 3 floats in [0, 1))
 *            element (row, column) of site m is kept when rng_uniform(seed + 0x9E3779B97F4A7C15 * call + *tick, (m << 40) + row *
 *            f_m + column) >= p_drop[m] (csrc/common.h; row counts through the WHOLE split) and scaled by 1 / (1 - p_drop[m]); tick
 *            is an optional device word (8-byte aligned; null: 0) that a captured graph can advance between replays.  With
 *            train == 0 or p_drop[m] == 0 the site is the identity and draws nothing
 *   params   host array of 32 DEVICE pointers to the module's own tensors (torch layouts, contiguous fp32; the LSTM weights
 *            16-byte aligned, the rest 4), per modality m = l, a, v at 10 * m: 0-3 encoder_m.lstm weight_ih, weight_hh, bias_ih,
 *            bias_hh; 4-5 encoder_m.fc1 weight, bias; 6-9 z<m>_to_f<m> fc1 weight, bias, fc2 weight, bias.  Then 30-31: fs_to_y
 *            weight, bias
 *   grads    host array of 32 DEVICE pointers (4-byte aligned) in the order of params, each the size of its parameter; null: the
 *            parameter is frozen, its products are skipped and nothing is written for it
 *   accumulate 0: the gradients are stored; 1: added to what grads holds.  Either way the chunks of one call add up in chunk order
 *   y_hat    [N, output_dim];  loss  1 float, written behind the last chunk
 *   max_rows row cap: chunks of at most max_rows rows (0: one chunk) that share the workspace
 *   workspace mfm_train_ablation_d_workspace_floats(T, N, sizes, max_rows) floats, 16-byte aligned, contents arbitrary; with rows =
 *            min(N, max_rows), Hp(h) = round_up(h, 16) and up4 = round_up(., 4), in this order: with rows < N up4(T * rows * D) for
 *            the chunk's copy of x; rows * T * 4 * (Hp(zl) + Hp(za) + Hp(zv)) gate records, each LSTM's [T, n, 4, Hp] for a chunk
 *            of n rows; rows * T * (Hp(zl) + Hp(za) + Hp(zv)) hidden states and as many cell states; up4(rows * zl) + up4(rows *
 *            za) + up4(rows * zv) for d h_T; the DROPOUT SCALES of the last chunk, up4(rows * (fl + fa + fv)): site m begins at
 *            rows * (the f sizes in front of it) and holds [n, f_m] row-major floats, 0 or 1 / (1 - p) -- written for the sites
 *            that draw, left alone otherwise; one partial of round_up(sum over the ten linears of out * in + out, 4) floats per
 *            workgroup, ceil(rows / tile rows) of them; up4(rows) loss contributions; up4(rows * T) ones (the bias gradients'
 *            right-hand side); and 4 floats for the fp64 running sum of the loss and the ticket word
 * mfm_train_ablation_d_mask_offset: host only; the first float of the dropout scales in that workspace (0 for bad sizes).
 * mfm_train_ablation_d_tile_rows: host only; rows per workgroup of the head kernel (tile_rows[0]), chosen as
 * mfm_predict_ablation_tile_rows chooses them: 1 while three workgroups per row stay below six per CU, else 4.
 * Nothing outside the workspace, y_hat, loss and the non-null gradients is written.  Any N >= 1 (< 2^24), T >= 1.  Sizes that do
 * not fit on chip -- a z_m or an f_m above 128 (MFM_SEQ_MAX_RESIDENT_H of the recurrences and the head's bound), or a head row
 * whose output_dim does not fit the LDS beside the rest -- return MFM_ERR_UNSUPPORTED with the size in the error text and enqueue
 * nothing: compose the granular entries instead.  Bad arguments (T or N < 1, N >= 2^24, a null pointer other than tick and the
 * entries of grads, a misaligned one, max_rows < 0, an unknown loss_kind, accumulate or train outside {0, 1}, a p_drop outside
 * [0, 1)) return MFM_ERR_ARG and enqueue nothing.  Stream-ordered, no host synchronisation, no allocation; legal inside a stream
 * capture on the one given stream (no forked branches). */
int64_t mfm_train_ablation_d_workspace_floats(int32_t T, int64_t N, const int32_t* sizes /*host, 12*/, int64_t max_rows); /* host only; 0 for bad sizes */
int64_t mfm_train_ablation_d_mask_offset(int32_t T, int64_t N, const int32_t* sizes /*host, 12*/, int64_t max_rows); /* host only */
int mfm_train_ablation_d_tile_rows(int64_t N, int64_t max_rows, int32_t* tile_rows /*host, 1*/);
int mfm_train_ablation_d(int32_t T, int64_t N, const int32_t* sizes /*host, 12*/, int32_t loss_kind, int32_t train,
                         const float* p_drop /*host, 3*/, uint64_t seed, uint64_t call, const uint64_t* tick /*device, or null*/,
                         const float* const* params /*host, 32*/, float* const* grads /*host, 32; null entries: frozen*/,
                         int32_t accumulate, const float* x, const void* y, float* workspace, float* y_hat, float* loss,
                         int64_t max_rows, void* stream);

/* ------------------------------------------------------------------------------------------
 * Prediction of the ablations M_A and M_C (csrc/ablation_mfn.hip; the same `evaluate` / `predict` blocks of the reference's
 * train_mfm_ablation, reference mfm_model.py:201-266 and :337-387): the two ablations whose label factor comes from the Memory
 * Fusion Network, under the contract of mfm_predict_ablation -- fp32, dropout the identity, no MfmPlan, no training workspace, no
 * x_hat written, no MMD:
 *   family 0, M_A   zy = last_to_zy_fc1(MFN(x)), fy = relu(zy_to_fy_fc2(relu(zy_to_fy_fc1(zy)))), y_hat = fy_to_y_fc2(relu(fy_to_y_fc1(fy)))
 *                   as mfm_predict_mfn computes them; zl = encoder_l(x) over ALL D columns of x, fl = relu(zl_to_fl_fc2(relu(
 *                   zl_to_fl_fc1(zl)))); gen_m = mean((decoder_m([fy | fl], T) - x_m)^2) for m in l, a, v
 *   family 1, M_C   the same label path; gen_m = mean((decoder_m(fy, T) - x_m)^2)
 * Per row chunk of n rows, on the one stream given: ONE grouped fp32 GEMM for the input projections (the MFN's three LSTMs on
 * their column ranges, and with gen family 0's encoder_l on all of x); ONE launch of (LSTM, row tile) workgroups -- an MFN LSTM
 * stores its cell states and last hidden state, encoder_l goes on with its fc1 and the zl -> fl MLP on chip and stores its fl
 * rows into columns [fy, fy + fl) of the chunk's embedding block [n, fy + fl] in the workspace (zl is never written); the
 * attention chain of mfm_encode_mfn; the memory recurrence with the label tail of mfm_predict_mfn (y_hat, one loss contribution
 * per row, the chunk's arrival ticket: the workgroup that draws the last ticket of a chunk adds the contributions in fp64 in a
 * fixed order and puts the ticket word back to 0), which with gen also stores the row's fy into columns [0, fy) of the
 * embedding block; with gen ONE launch of (decoder m, row tile) workgroups that all stage the same embedding rows and store
 * h_t, the decoders' fc1 fused with the squared error, one partial per workgroup, and one workgroup that adds the partials in
 * fp64 in a fixed order.  No workgroup waits for another, the loss ticket is the only ticket, no float atomics touch a result.
 * With with_gen 0 encoder_l, its projection and the decoders do not run and their parameters are not read.
 *   sizes    host, 23: the layout of mfm_predict_zeros_mfn (d_l, d_a, d_v; zl, za, zv; zy; h_l, h_a, h_v; memsize; windowsize; the
 *            hidden widths of att1, att2, gamma1, gamma2; heads; fl, fa, fv, fy, output_dim, loss_kind).  Entries a family does not
 *            have may be any positive value: za, zv, fa, fv, and for M_C also zl and fl; heads must be 0 or 1 and is unused.
 *            loss_kind 0: L1 against float labels y [N, output_dim]; 1: cross entropy against int64 class indices y [N]
 *   with_gen 1: gen is computed and must not be null; 0: gen must be null, neither encoder_l nor a decoder runs
 *   params   host array of 66 DEVICE pointers to the module's own tensors (torch layouts, contiguous fp32; the LSTM weights
 *            16-byte aligned, the rest 4).  0-37, the 38 of mfm_predict_mfn in its offset order: per MFN LSTM l, a, v weight_ih,
 *            weight_hh, bias_ih, bias_hh (12); weight and bias of att1_fc1, att1_fc2, att2_fc1, att2_fc2, gamma1_fc1, gamma1_fc2,
 *            gamma2_fc1, gamma2_fc2 (16); of last_to_zy_fc1 (2); of zy_to_fy_fc1, zy_to_fy_fc2, fy_to_y_fc1, fy_to_y_fc2 (8).
 *            38-55: decoder_l, decoder_a, decoder_v, each lstm weight_ih, weight_hh, bias_ih, bias_hh, fc1 weight, bias (hidden size
 *            fy + fl for M_A, fy for M_C) -- not read, and may be null, when with_gen is 0.  56-65: encoder_l lstm weight_ih (over
 *            all D columns), weight_hh, bias_ih, bias_hh, fc1 weight, bias, then zl_to_fl fc1 weight, bias, fc2 weight, bias -- not
 *            read, and may be null, when with_gen is 0 or family is 1
 *   x        [T, N, D] time-major and contiguous, D = d_l + d_a + d_v, 4-byte aligned: any contiguous view; read only
 *   y        labels of the whole split, or null: no label loss (then disc must be null too)
 *   y_hat    [N, output_dim];  gen  3 floats in the order l, a, v;  disc  1 float, the mean over the WHOLE split whatever the
 *            chunking; gen and disc are written behind the last chunk
 *   max_rows row cap: chunks of at most max_rows rows (0: one chunk) that share the workspace
 *   workspace mfm_predict_ablation_mfn_workspace_floats(T, N, sizes, family, with_gen, with_labels, max_rows) floats, 16-byte
 *            aligned, contents arbitrary.  With rows = min(N, max_rows), Hp(h) = round_up(h, 16), up4(v) = round_up(v, 4),
 *            w = fy + fl (M_A) or fy (M_C), in this order:
 *              rows * T * 4 * (Hp(h_l) + Hp(h_a) + Hp(h_v))                                   the MFN's x-projections
 *            + rows * T * 4 * Hp(zl)                          (M_A with gen)                  encoder_l's x-projection
 *            + rows * T * (Hp(h_l) + Hp(h_a) + Hp(h_v))                                       the MFN LSTMs' cell states
 *            + up4(rows * h_l) + up4(rows * h_a) + up4(rows * h_v)                            their last hidden states
 *            + up4(rows * T * memsize) + up4(rows * T * gamma1) + up4(rows * T * gamma2)      cHat, the gamma partials
 *            + up4(rows * w)                                                                  the embedding block
 *            + 3 * rows * T * Hp(w)                           (with gen)                      the decoders' stored h
 *            + up4(sum over m of ceil(T * rows / 64) * ceil(d_m / 64))   (with gen)           the squared-error partials
 *            + 12                                             (with gen)                      six fp64 accumulators
 *            + up4(rows)                                      (with labels)                   one loss contribution per chunk row
 *            + 4                                                                              the fp64 running sum, the ticket word, a pad
 *            It does not grow with N beyond the row cap.  With labels the call clears the ticket word itself (a memset on the
 *            stream) and leaves it at 0: it is the third of the last four floats.
 * mfm_predict_ablation_mfn_tile_rows: host only; rows per workgroup of the recurrence launch (tile_rows[0]) and of the decoders'
 * ([1]; 0 without gen): 1 below six workgroups per CU over a launch of three LSTMs, else 4.  The recurrence launch counts the
 * MFN's three LSTMs alone, with and without gen: y_hat and disc have the same bits with and without gen.  Results are
 * bit-identical from call to call; y_hat also across row caps that keep the tile rows (gen and disc then differ in the grouping
 * of the fp64 sums alone).
 * Nothing outside the workspace and the three outputs is written.  MFM_ERR_UNSUPPORTED with the size in the error text, nothing
 * enqueued: what mfm_predict_mfn refuses (an h_dims entry above 128, a windowsize other than 2, attention widths beyond the LDS,
 * memsize or gamma widths beyond the register-resident memory recurrence, a label tail beyond the LDS); with gen zl > 128 (M_A),
 * a decoder width fy + fl (M_A) or fy (M_C) above 128, or more LDS than a CU has: compose the granular entries instead.  Bad
 * arguments (T or N < 1, N >= 2^24, a size below 1, a null pointer, y without disc or disc without y, gen without with_gen or
 * with_gen without gen, max_rows < 0, a family outside {0, 1}) return MFM_ERR_ARG and enqueue nothing.  Stream-ordered, no host
 * synchronisation, no allocation; legal inside a stream capture on the one given stream (no forked branches). */
int64_t mfm_predict_ablation_mfn_workspace_floats(int32_t T, int64_t N, const int32_t* sizes /*host, 23*/, int32_t family, int32_t with_gen,
                                                  int32_t with_labels, int64_t max_rows); /* host only; 0 for bad sizes */
int mfm_predict_ablation_mfn_tile_rows(int64_t N, int32_t family, int32_t with_gen, int64_t max_rows, int32_t* tile_rows /*host, 2*/);
int mfm_predict_ablation_mfn(int32_t T, int64_t N, const int32_t* sizes /*host, 23*/, int32_t family, int32_t with_gen,
                             const float* const* params /*host, 66*/, const float* x, const void* y /*null: no label loss*/,
                             float* workspace, float* y_hat, float* gen /*3, or null*/, float* disc /*1, or null*/, int64_t max_rows,
                             void* stream);

/* ------------------------------------------------------------------------------------------
 * Gradient all-reduce of the data-parallel step (the reference has no multi-GPU
 * path): in-place fp32 sum of one flat buffer over all ranks of one node, ONE kernel launch on the
 * caller's stream, no host synchronisation.  Ranks are one process per GPU; every rank owns an uncached
 * staging block that its peers map through HIP IPC and write over xGMI (two-shot: scatter-reduce + gather,
 * csrc/p2p.hip).  Every slice is summed once, by its owner, in rank order: all ranks receive bit-identical
 * results.  Set-up: create on every rank -> export 64-byte handle -> exchange the handles out of band
 * (factorized_amd/comm.py uses torch.distributed.all_gather_object) -> connect -> barrier.
 * Waits inside the kernel are bounded (MFM_P2P_TIMEOUT_MS, default 10000): a missing peer raises the
 * flag read by mfm_p2p_status instead of hanging the device. */
int mfm_p2p_create(int32_t nranks /*<=8*/, int32_t rank, int64_t max_elems, void** handle);
int mfm_p2p_handle_bytes(void);
int mfm_p2p_export(void* handle, void* out /*mfm_p2p_handle_bytes()*/);
int mfm_p2p_connect(void* handle, const void* all_handles /*nranks x mfm_p2p_handle_bytes(), rank order*/);
/* ranks that live in ONE process (one host thread / stream per GPU with peer access enabled, or several
 * streams of one GPU in tests) skip IPC: hand every rank the others' local base pointers */
void* mfm_p2p_local_base(void* handle);
int mfm_p2p_connect_bases(void* handle, const void* const* bases /*nranks, rank order; own entry ignored*/);
int mfm_p2p_allreduce(void* handle, float* buf /*16-byte aligned*/, int64_t n /*<= max_elems*/, void* stream);
/* the same exchange with the flat Adam update (mfm_adam_flat semantics) applied by the rank-local copy of the
 * kernel as each reduced slice arrives: all-reduce + optimizer in one launch.  `grads` still receives the sum. */
int mfm_p2p_allreduce_adam(void* handle, float* grads, float* p, float* m, float* v, int64_t n, int32_t step,
                           float lr, float beta1, float beta2, float eps, float grad_scale, void* stream);
/* ABI 3: the same with a guard word (mfm_adam_flat_guarded): element `guard_index` of `grads` (-1: none).  A rank whose guard
 * is raised says so in its first-push flags; every rank then completes the exchange (the sum carries the NaN too) but NO rank
 * touches p, m, v -- the replicas skip the same steps and stay bit-identical. */
int mfm_p2p_allreduce_adam_guarded(void* handle, float* grads, float* p, float* m, float* v, int64_t n, int32_t step,
                                   float lr, float beta1, float beta2, float eps, float grad_scale, int64_t guard_index,
                                   void* stream);
int mfm_p2p_status(void* handle, int32_t* timed_out /*1 if any wait gave up since create (synchronises)*/);
/* diagnosis of a sub-par scaling run: ticks (100 MHz wall clock) workgroup 0 of THIS rank spent spinning in flag round 1 (the
 * peers' first pushes) and round 2 (the owners' results), summed over the exchanges since create / the last reset, and the
 * number of exchanges: out[0], out[1], out[2] (synchronises; bench.py --gpus N prints them per rank) */
int mfm_p2p_wait_stats(void* handle, int64_t* out /*[3]*/, int32_t reset);
void mfm_p2p_destroy(void* handle);

/* ------------------------------------------------------------------------------------------
 * The fused MFM_KL_EF training / inference plan (mfm_model.py:557-660 + mfm_mosi.py:424-442).
 * One call enqueues the whole step: input projections -> 4 encoder recurrences -> latent
 * heads/MLPs/classifier + KLD + L1|CE -> 3 decoder recurrences -> fc1 + MSE -> full backward
 * -> (optional) Adam.  Parameters live in ONE flat fp32 buffer; `param_offsets` gives the
 * element offset of each of the MFM_KLEF_NPARAM tensors in reference state_dict order
 * (encoder_l.lstm.weight_ih ... fy_to_y_fc2.bias; 78 tensors).
 */
#define MFM_KLEF_NPARAM 78
#define MFM_LOSS_SLOTS 8  /* [0]=disc [1]=mse_l [2]=mse_a [3]=mse_v [4]=kld [5]=total loss */

typedef struct MfmPlanConfig {
  int32_t d_l, d_a, d_v;
  int32_t zl, za, zv, zy;
  int32_t fl, fa, fv, fy;
  int32_t output_dim;
  int32_t loss_kind;      /* 0 = L1 (mfm_mosi.py:411,438), 1 = cross-entropy (mfm_you.py:451,484) */
  int32_t T, B;
  float lda_xl, lda_xa, lda_xv, lda_reg;   /* mfm_mosi.py:433,437 */
  float drop_zy, drop_zl, drop_za, drop_zv, drop_y;
  float reg_scale;        /* extra factor on the KLD term (DP: world size) */
  int32_t precision;      /* 0 = fp32 everywhere (BASELINE config 1; 1e-4 parity with the reference);
                             1 = bf16 MFMA operands in every GEMM and LSTM recurrence, fp32 accumulation, master
                                 weights, Adam moments, cell state, saved activations, latent stack and losses
                                 (BASELINE configs 2-4; gate: matched loss curve) */
  /* ---- model variant (the classes train_mfm picks by config['type'], reference mfm_mosi.py:398-401) */
  int32_t variant;        /* 0 = MFM_KL_EF (early-fusion LSTM for z_y; mfm_model.py:557-660)
                             1 = MFM_KL    (Memory Fusion Network for z_y + KLD;  mfm_model.py:662-764, 93-199)
                             2 = MFM       (MFN for z_y, no logvar heads, MMD regulariser; mfm_model.py:469-555, 14-34) */
  int32_t hl, ha, hv;     /* variants 1, 2: MFN LSTMCell sizes (config["h_dims"]) */
  int32_t mem_dim;        /* memsize; windowsize is 2 (cStar = [c_{t-1}, c_t]) */
  int32_t nn1, nn2, g1, g2;                       /* hidden widths of att1 / att2 / gamma1 / gamma2 (*Config["shapes"]) */
  float drop_nn1, drop_nn2, drop_g1, drop_g2;     /* their dropouts (*Config["drop"]) */
} MfmPlanConfig;

typedef struct MfmPlan MfmPlan;

/* number of parameter tensors of a variant in reference state_dict order: 78 / 104 / 90 */
int mfm_plan_num_params(int32_t variant);
/* host-side: builds the op tables; no device allocation.  param_offsets has mfm_plan_num_params(cfg->variant)
 * entries: the element offset of every tensor of the reference model's state_dict(), in its order, inside the
 * flat buffer (the MFN's out_fc1 / out_fc2 exist in the state_dict but are unused by forward, as in the reference). */
int mfm_plan_create(const MfmPlanConfig* cfg, const int64_t* param_offsets /*[mfm_plan_num_params(variant)]*/,
                    int64_t n_params_total, MfmPlan** out);
/* variant 2 only: the N(0,1) sample loss_MMD draws for every forward (reference mfm_model.py:26: torch.randn on the
 * host).  [B, zl+za+zv+zy] row-major device buffer read by the next forward / step calls; the caller refreshes it
 * (or keeps it fixed for parity runs). */
int mfm_plan_set_gauss(MfmPlan* plan, const float* gauss);
void mfm_plan_destroy(MfmPlan* plan);
int64_t mfm_plan_workspace_bytes(const MfmPlan* plan);

/* zero the workspace and write its constant regions (a ones vector used for bias-gradient
 * column sums).  Call once after allocating `workspace` (and again if it is re-allocated). */
int mfm_plan_init_workspace(MfmPlan* plan, void* workspace, void* stream);

/* Forward only (evaluate/predict, mfm_mosi.py:445-465; also the first half of a step).
 * x [T,B,D] time-major contiguous, y [B] (L1, output_dim 1) / [B,output_dim] (L1) / int64 [B] (CE).
 * train!=0 applies dropout with the counter-based generator keyed by (seed, call counter).
 * Outputs (any may be NULL): xhat_l/a/v [T,B,d_*], y_hat [B,output_dim], losses[MFM_LOSS_SLOTS]. */
int mfm_plan_forward(MfmPlan* plan, const float* params, const float* x, const void* y, int train,
                     uint64_t seed, void* workspace, float* xhat_l, float* xhat_a, float* xhat_v,
                     float* y_hat, float* losses, void* stream);

/* Backward of the last mfm_plan_forward on the same workspace: fills grads (same flat layout,
 * zeroed first).  stage: 0 joint loss (mfm_mosi.py:439), 1 gen+reg, 2 disc+reg (train_beta_vae,
 * mfm_mosi.py:278-281). */
int mfm_plan_backward(MfmPlan* plan, const float* params, const float* x, const void* y, int stage,
                      void* workspace, float* grads, void* stream);

/* Backward of the last mfm_plan_forward for ARBITRARY upstream gradients (the autograd path of the
 * nn.Module mirror: the caller's own loss.backward(), mfm_mosi.py:440): d_xhat_* [T,B,d_*],
 * d_yhat [B,output_dim], d_reg = device scalar dLoss/dKLD. */
int mfm_plan_backward_ext(MfmPlan* plan, const float* params, const float* x, const float* d_xhat_l,
                          const float* d_xhat_a, const float* d_xhat_v, const float* d_yhat,
                          const float* d_reg, void* workspace, float* grads, void* stream);

/* ---- the module path's LAZY losses (round 5).  The reference's loop (mfm_mosi.py:427-441) calls model.forward(batch_X), then
 * builds  loss = L1(y_hat, y) + sum_m lda_m MSE(x_hat_m, x_m) + lda_mmd * reg  from the outputs and calls loss.backward().
 * The plan's forward already holds the three MSE terms, the regulariser and lda_m-scaled d x_hat (decoder fc1 epilogue): when
 * the loop's loss is exactly such a weighted sum (factorized_amd/lazy.py recognises it), no x_hat tensor, no torch loss kernel
 * and no autograd graph is needed:
 *   mfm_plan_forward_train     = mfm_plan_forward(train=1, y=NULL, no outputs): x_hat / y_hat stay in the workspace
 *                                (mfm_plan_out_layout), the loss slots [1..4] are filled, slot [0] stays 0; `grads_to_zero`
 *                                (optional, the plan's flat layout) is cleared inside the first launch.
 *   mfm_plan_backward_weighted = backward of  w.disc * L_disc(y_hat, y) + sum_m w.gen_m * MSE_m + w.reg * reg  on the last
 *                                forward.  w.gen_* must equal the plan's lda_x* or all be 0 (MFM_ERR_UNSUPPORTED otherwise:
 *                                the caller falls back to mfm_plan_backward_ext); write_disc_loss != 0 adds L_disc into loss
 *                                slot [0] (the forward ran without labels).  `grads` is overwritten (cleared first unless
 *                                this step's forward_train already cleared it). */
typedef struct MfmLossWeights { float disc, gen_l, gen_a, gen_v, reg; int32_t write_disc_loss; } MfmLossWeights;
int mfm_plan_forward_train(MfmPlan* plan, const float* params, const float* x, uint64_t seed, void* workspace,
                           float* grads_to_zero, void* stream);
int mfm_plan_backward_weighted(MfmPlan* plan, const float* params, const float* x, const void* y,
                               const MfmLossWeights* w /*host*/, void* workspace, float* grads, void* stream);
/* byte offsets inside the workspace of x_hat_l / x_hat_a / x_hat_v [T,B,d_*] (out[0..2]; -1 on bf16-resident plans, which
 * do not keep them) and y_hat [B,output_dim] (out[3]) as the last forward left them; out[4..7] reserved (-1) */
int mfm_plan_out_layout(const MfmPlan* plan, int64_t* out /*[8]*/);

/* forward (train mode) + backward of the joint loss in one enqueue, no optimizer: the data-parallel step
 * all-reduces `grads` next and then calls mfm_adam_flat (factorized_amd/train.py).  Same launches as
 * mfm_plan_train_step minus Adam; the gradient buffer is cleared inside the first launch. */
int mfm_plan_grad_step(MfmPlan* plan, const float* params, float* grads, const float* x, const void* y,
                       uint64_t seed, void* workspace, float* losses, void* stream);

/* forward + backward + Adam in one enqueue (no host work in between). */
int mfm_plan_train_step(MfmPlan* plan, float* params, float* grads, float* adam_m, float* adam_v,
                        const float* x, const void* y, uint64_t seed, int32_t step, float lr,
                        float grad_scale, void* workspace, float* losses, void* stream);

/* forward (train mode) + backward of the STAGE loss (0 joint, 1 gen+reg, 2 disc+reg) + Adam over `spans`
 * (mfm_adam_flat_spans semantics) in one enqueue: one step of train_beta_vae's loop (reference mfm_mosi.py:255-285). */
int mfm_plan_train_step_staged(MfmPlan* plan, float* params, float* grads, float* adam_m, float* adam_v,
                               const float* x, const void* y, uint64_t seed, int32_t stage,
                               const MfmAdamSpan* spans /*host*/, int32_t nspans, float lr, float grad_scale,
                               void* workspace, float* losses, void* stream);

/* ---- per-plan switches (ABI 3).  Everything a plan decides is decided from its sizes; these are the switches a caller (or
 * a test) may set explicitly.  Unknown keys return MFM_ERR_ARG.
 *   "handover"            1 (default): B <= 32 plans of MFM_KL_EF run their input projections and weight gradients on role
 *                         workgroups INSIDE the encoder launches (in-launch hand-overs; the launch needs the GPU to itself).
 *                         0: separate launches, no workgroup ever waits for another one.  The host flips it to 0 when a
 *                         hand-over timed out (mfm_plan_status) or when several ranks share one device.
 *   "handover_timeout_us" how long a consumer spins before it gives up (default 50000).
 *   "grad_guard_offset"   element offset inside the gradient buffer of the guard word of mfm_adam_flat_guarded (default -1:
 *                         none; a wait that gives up then stores its NaN into grads[0]).  With an offset set, the plan's own
 *                         Adam launches are guarded, and every backward stores a NaN there while the status word is non-zero.
 *   "bf16_dot"            bf16 plans at batch sizes below the bf16 MFMA recurrences (B < 192): 1 = the one-row recurrences
 *                         that have the variant take their recurrent product on bf16 dot products (MfmSeqDesc::bf16_dot);
 *                         default 0 (measured: profiles/r04_bf16_onerow.txt; MFM_BF16_DOT=1 sets the default for new plans).
 *   "inject_fault"        fault injection for tests, one shot: 1 = one projection producer of the next forward does not raise
 *                         its flag; 2 = one BPTT workgroup of the next backward does not stamp its last gate gradients.
 *                         The waiting side must time out, set the status word and poison the guard. */
int mfm_plan_set_option(MfmPlan* plan, const char* key, int64_t value);
/* The tuning / test switches named MFM_* ("Kernel selection and its overrides") belong to the PLAN: its table is
 * filled from the environment when the plan is created and consulted -- never the environment -- by every launch the plan
 * issues.  This call changes one entry afterwards (value NULL removes it); switches that shape the workspace (MFM_BF16_STORE,
 * MFM_LATENT_*, ...) are read at creation only.  The granular entry points of this header, which have no plan, read the
 * environment at each call. */
int mfm_plan_set_option_str(MfmPlan* plan, const char* key, const char* value);
/* also answers three read-only keys: "proj_roles_active" / "dw_roles_active" = 1 when the plan's last forward / backward ran on
 * role workgroups; "dw_f32_items" = the number of LSTMs whose weight gradients the last backward took on the fp32 one-pass
 * kernel (MFM_DW_F32_MINROWS; 0: all on the GEMMs) */
int mfm_plan_get_option(const MfmPlan* plan, const char* key, int64_t* value);

/* Device-side state of a plan inside its workspace: out[0] byte offset of the plan's own loss slots [MFM_LOSS_SLOTS] floats
 * (used when `losses` is NULL), out[1] byte offset of the STATUS word (uint32, right behind them: 0 = fine; bit 0 a consumer of
 * projections gave up waiting, bit 1 a weight-gradient block did; sticky -- only the host clears it, mfm_plan_clear_status),
 * out[2] byte offset of the replay counter (uint64) and out[3] of the backward replay counter (uint32): device words a
 * captured hipGraph advances on every replay (the dropout streams and the hand-over epochs add them), out[4..7] reserved. */
int mfm_plan_state_layout(const MfmPlan* plan, int64_t* out /*[8]*/);
/* The same failure, visible WITHOUT a copy or a synchronisation: two uint32 words of host-coherent pinned memory owned by the
 * plan (allocated by mfm_plan_init_workspace; NULL before).  A consumer that gives up stores 1 into word [0] (projections) /
 * 2 into word [1] (weight gradients) with a system-scope store next to the device status word; an optimizer polls them for
 * free before every update (factorized_amd/optim.py).  mfm_plan_clear_status clears them too. */
int mfm_plan_host_status(MfmPlan* plan, uint32_t** out /*host pointer*/);
/* enqueue the clearing of the status word */
int mfm_plan_clear_status(MfmPlan* plan, void* workspace, void* stream);

/* Where the latent stack keeps its per-row record inside the workspace (tests and tuning aids: dropout masks and
 * pre-activation gradients can be read back from the workspace tensor).  out[0] byte offset of the activation
 * record [B, rec], out[1] byte offset of the gradient record, out[2] rec (floats per row); then record offsets
 * (floats): out[3..6] dropout scale (0 or 1/(1-p)) of z{l,a,v,y}_to_f*_fc1, out[7] of fy_to_y_fc1,
 * out[8..11] post-dropout activation of the same four layers, out[12] of fy_to_y_fc1, out[13..16] their widths
 * f{l,a,v,y}, out[17..20] f segments (outputs of *_fc2), out[21] y_hat, out[22] 1 if the row-per-workgroup kernels
 * run at this (T,B), out[23..26] mu segments z{l,a,v,y} (inputs of *_fc1), out[27..30] their widths, out[31] reserved. */
int mfm_plan_latent_layout(const MfmPlan* plan, int64_t* out /*[32]*/);
/* Which kernel form the latent stack takes at this plan's sizes and (T,B) (tests: a size matrix asserts the form it is there
 * for).  out[0] 1 = row-per-workgroup kernels, 0 = staged kernels; out[1] floats of the weight panel the staged kernels keep in
 * LDS (0: they read the weights from L2); out[2] rows per workgroup of the staged backward, out[3] of the staged forward;
 * out[4] 1 = the staged products run on the fp32 MFMA, 0 = quad form; out[5] workgroups per row of the row kernels (4: one per
 * modality chain, 1 otherwise); out[6] 1 = the row backward adds its bias gradients from the tabulated list, 0 = it searches
 * the op table (always 0 off the row path); out[7] stages; out[8] 1 = the early-fusion encoder's fc1 has a stage of its own;
 * out[9] floats per row record; out[10] / out[11] the largest K / N of a layer; out[12] / out[13] work items of the widest
 * stage, forward (4 x sum of N) / backward (4 x sum of K); out[14] biases of all layers together; out[15] reserved. */
int mfm_plan_latent_form(const MfmPlan* plan, int64_t* out /*[16]*/);

/* variants 1, 2: where the Memory Fusion Network keeps its [T*B, .] tensors inside the workspace (tests / tuning aids).
 * Byte offsets: out[0] cStar, out[1] h1 = drop(relu(att1_fc1)), out[2] its relu/dropout mask (0 | 1/(1-p)), out[3] attention,
 * out[4] attended, out[5] h2, out[6] its mask, out[7] cHat, out[8] final memory [B, memsize], out[9] the latent stack's y
 * input [B, nzy]; then sizes: out[10] width of cStar, out[11] NN1, out[12] NN2 hidden widths, out[13] memsize, out[14] nzy,
 * out[15] T*B. */
int mfm_plan_mfn_layout(const MfmPlan* plan, int64_t* out /*[16]*/);

/* Where LSTM `which` keeps its saved activations inside the workspace (tests / tuning aids).  which: 0 .. n_enc-1 the
 * encoders in plan order (l, a, v, early-fusion | l, a, v, MFN l, a, v), then the three decoders.  Byte offsets out[0] gates
 * [T,B,4,Hp], out[1] hs [T,B,Hp], out[2] cs [T,B,Hp] (always fp32); out[3] h, out[4] Hp; out[5] 1 when the plan is
 * bf16-RESIDENT: gates, hs, the decoders' dH and d x_hat are __bf16 buffers; out[6] 1 for a decoder; decoders: out[7] dH
 * [T,B,Hp], out[8] d x_hat [T*B, out[9]] (out[10] real columns); encoders: out[7] the fp32 copy of h_{T-1} [B,Hp] (-1: none);
 * out[11] 1 when the recurrences run on the bf16 MFMA kernels. */
int mfm_plan_seq_layout(const MfmPlan* plan, int32_t which, int64_t* out /*[12]*/);
/* The kernel family of LSTM `which` (numbered as above): out[0] 0 = weight-resident recurrence kernels, 1 = step-by-step path
 * (recurrent GEMM + cell kernel per time step: h above out[1], or MFM_SEQ_STEPWISE set); out[1] the widest resident h;
 * out[2] 1 when a weight-resident fp32 recurrence runs on the MFMA kernels (16 rows per workgroup: B above 512, or
 * MFM_SEQ_PATH), 0 on the VALU kernels, the step-by-step path or the bf16 kernels; out[3] reserved. */
int mfm_plan_seq_form(const MfmPlan* plan, int32_t which, int64_t* out /*[4]*/);

/* Algorithmic work of one training step at this plan's (T,B):
 * 3 x forward FLOPs; activation+input bytes per sample plus 10 P 4 parameter/optimizer bytes. */
double mfm_plan_flops_per_step(const MfmPlan* plan);
double mfm_plan_bytes_per_step(const MfmPlan* plan);

/* Per-kernel timing with HIP events recorded on the launch stream (bench.py's roofline object).
 * mask bit k enables kernel id k (ids 0..mfm_plan_num_kernels()-1, names from
 * mfm_plan_kernel_name); mfm_plan_collect_timing synchronises on the recorded events, returns
 * summed milliseconds and launch counts per kernel id and resets the recorder. */
int mfm_plan_set_timing(MfmPlan* plan, int mask);
/* bracket only every `every`-th step (default 1 = every step): an event bracket is two extra packets on the stream
 * (mfm_timing_bracket_overhead_ms), which a timed region should not pay on every step */
int mfm_plan_set_timing_every(MfmPlan* plan, int every);
int mfm_plan_num_kernels(void);
const char* mfm_plan_kernel_name(int kid);
int mfm_plan_collect_timing(MfmPlan* plan, double* sum_ms, int64_t* count);
/* median cost (ms) of an EMPTY event bracket on `stream`: what a bracket adds to the kernel it surrounds */
int mfm_timing_bracket_overhead_ms(void* stream, double* ms_out);
/* algorithmic FLOPs of ONE launch of kernel `kid` (matrix work only). */
double mfm_plan_kernel_flops(const MfmPlan* plan, int kid);

#ifdef __cplusplus
}
#endif
#endif /* MFM_HIP_H_ */
