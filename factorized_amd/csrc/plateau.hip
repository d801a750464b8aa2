// torch.optim.lr_scheduler.ReduceLROnPlateau.step on learning rates that live in device memory
// (factorized_amd.lr_scheduler.ReduceLROnPlateau; the reference's `scheduler.step(valid_loss)` at the end of every epoch,
// mfm_mosi.py:470-477): ONE launch reads a metric, advances the scheduler's state and, when the plateau rule says so, scales the
// fp32 lr words of up to MFM_PLATEAU_MAX_GROUPS parameter groups in place.  Metric, state and learning rates never reach the
// host, and a captured launch decides anew on every replay.
//
// The state block (MfmPlateauState, include/mfm_hip.h) lives in device memory: best (a double), num_bad_epochs,
// cooldown_counter, last_epoch, reduced (1: this launch changed at least one lr) and reductions (launches that did, so far).
// The metric is one device float (`metric_dev`) or, when that pointer is null, the double kernel argument `metric_host` (a
// python float keeps its 53 bits, as in torch).  The learning rates are reached through a table of pointers that travels by
// value in the kernel-argument segment; it is indexed by the loop counter of the one working lane, i.e. uniformly (scalar
// loads, no copy to scratch).
//
// The rule is torch 2.10's step / _is_better / _reduce_lr, statement for statement, in fp64 (plateau_rule below: each line
// names the python statement it restates).  torch evaluates the same expressions in python doubles and writes a tensor lr with
// fill_(new_lr), which rounds the double to fp32 to nearest even -- what `(float)new_lr` does -- so decisions, state and lr
// bits are IDENTICAL to torch's, not merely close.  That only holds while every product is rounded before it is used:
//     old_lr - max(old_lr * factor, min_lr)
// contracts to fma(-old_lr, factor, old_lr) under the device default (-ffp-contract=fast), whose unrounded product changes
// the comparison with eps in the last bit.  Hence `#pragma clang fp contract(off)` around the rule.  python's max(a, b) is
// `b > a ? b : a`; it is written that way rather than as fmax, which differs from it for a NaN lr (neither form writes one:
// `old_lr - new_lr > eps` is false for a NaN).  A NaN metric compares false in every _is_better form and counts as a bad
// epoch, as in torch.  Groups are walked in order by the one lane, so two groups that share one lr tensor are reduced twice,
// as by torch's loop; a launch that does not reduce stores no lr word at all.
//
// One workgroup of one wave; lane 0 does everything (a handful of dependent scalar operations: spreading them would only add
// a ticket), the other lanes leave at once.  Nothing waits or spins.  State loads and stores are relaxed agent-scope atomics
// (the KB_LOAD / KB_STORE style of keep_best.hip), the lr words move as plain loads and stores; the next launch on the stream
// starts behind the end of this one.  One launch at a time may use a state block.
//
// Compiler resource report (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage):
//   plateau_step_kernel   VGPRs 12   AGPRs 0   SGPRs 27  scratch 0 bytes   LDS 0 bytes   occupancy 8 waves/SIMD
// In the generated code the products and differences of the rule are separate v_mul_f64 / v_add_f64 (no v_fma_f64), the table
// is read with s_load_dwordx2 at a scalar offset, and every store is a vector store (global_store_dword / _dwordx2) from lane 0.
#include "internal.h"

namespace mfm {

#define PL_LOAD(ptr) __hip_atomic_load(ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define PL_STORE(ptr, v) __hip_atomic_store(ptr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

struct PlateauArgs {
  double factor, threshold, eps;
  int n_groups, mode, threshold_mode, patience, cooldown, epoch;
};

__device__ __forceinline__ void plateau_rule(MfmPlateauState* st, double current, const MfmPlateauGroups& tab,
                                             const PlateauArgs& a) {
#pragma clang fp contract(off)
  double best = PL_LOAD(&st->best);
  int num_bad_epochs = PL_LOAD(&st->num_bad_epochs);
  int cooldown_counter = PL_LOAD(&st->cooldown_counter);
  const int last_epoch = PL_LOAD(&st->last_epoch);
  const int reductions = PL_LOAD(&st->reductions);

  const int epoch = a.epoch == -1 ? last_epoch + 1 : a.epoch;          // if epoch is None: epoch = self.last_epoch + 1
  bool better;                                                         // self._is_better(current, self.best)
  if (a.mode == MFM_PLATEAU_MIN && a.threshold_mode == MFM_PLATEAU_REL) {
    const double rel_epsilon = 1.0 - a.threshold;
    better = current < best * rel_epsilon;
  } else if (a.mode == MFM_PLATEAU_MIN) {
    better = current < best - a.threshold;
  } else if (a.threshold_mode == MFM_PLATEAU_REL) {
    const double rel_epsilon = a.threshold + 1.0;
    better = current > best * rel_epsilon;
  } else {
    better = current > best + a.threshold;
  }
  if (better) {
    best = current;
    num_bad_epochs = 0;
  } else {
    num_bad_epochs += 1;
  }
  if (cooldown_counter > 0) {                                          // if self.in_cooldown:
    cooldown_counter -= 1;
    num_bad_epochs = 0;
  }
  int reduced = 0;
  if (num_bad_epochs > a.patience) {
    for (int i = 0; i < a.n_groups; ++i) {                             // self._reduce_lr(epoch)
      float* lr = tab.lr[i];
      const double old_lr = (double)*lr;                               // float(param_group["lr"])
      const double scaled = old_lr * a.factor, floor_lr = tab.min_lr[i];
      const double new_lr = floor_lr > scaled ? floor_lr : scaled;     // max(old_lr * self.factor, self.min_lrs[i])
      if (old_lr - new_lr > a.eps) {
        *lr = (float)new_lr;                                           // param_group["lr"].fill_(new_lr)
        reduced = 1;
      }
    }
    cooldown_counter = a.cooldown;
    num_bad_epochs = 0;
  }
  PL_STORE(&st->best, best);
  PL_STORE(&st->num_bad_epochs, num_bad_epochs);
  PL_STORE(&st->cooldown_counter, cooldown_counter);
  PL_STORE(&st->last_epoch, epoch);
  PL_STORE(&st->reduced, reduced);
  PL_STORE(&st->reductions, reductions + reduced);
}

__global__ __launch_bounds__(64) void plateau_step_kernel(MfmPlateauState* st, const float* metric_dev, double metric_host,
                                                          MfmPlateauGroups tab, PlateauArgs a) {
  if (threadIdx.x != 0) return;
  const double current = metric_dev ? (double)PL_LOAD(metric_dev) : metric_host;      // current = float(metrics)
  plateau_rule(st, current, tab, a);
}

int plateau_step_launch(MfmPlateauState* state, const float* metric_dev, double metric, const MfmPlateauGroups* groups,
                        int n_groups, int mode, int threshold_mode, double factor, double threshold, double eps, int patience,
                        int cooldown, int epoch, hipStream_t stream) {
  static const char* who = "plateau step";
  MFM_REQUIRE(state && groups, "%s: bad arguments (state and groups must not be null)", who);
  MFM_REQUIRE(((uintptr_t)state & 15) == 0 && ((uintptr_t)metric_dev & 3) == 0,
              "%s: state must be 16-byte aligned (an MfmPlateauState) and the device metric 4-byte aligned", who);
  MFM_REQUIRE(n_groups >= 1 && n_groups <= MFM_PLATEAU_MAX_GROUPS, "%s: n_groups %d (1..%d)", who, n_groups,
              MFM_PLATEAU_MAX_GROUPS);
  MFM_REQUIRE(mode == MFM_PLATEAU_MIN || mode == MFM_PLATEAU_MAX, "%s: unknown mode %d", who, mode);
  MFM_REQUIRE(threshold_mode == MFM_PLATEAU_REL || threshold_mode == MFM_PLATEAU_ABS, "%s: unknown threshold mode %d", who,
              threshold_mode);
  MFM_REQUIRE(!(factor >= 1.0), "%s: factor %g (Factor should be < 1.0.)", who, factor);
  MFM_REQUIRE(patience >= 0 && cooldown >= 0, "%s: patience %d, cooldown %d (must not be negative)", who, patience, cooldown);
  MfmPlateauGroups tab;
  memset(&tab, 0, sizeof(tab));
  for (int i = 0; i < n_groups; ++i) {
    MFM_REQUIRE(groups->lr[i] && ((uintptr_t)groups->lr[i] & 3) == 0, "%s: lr pointer of group %d is null or not 4-byte aligned",
                who, i);
    tab.lr[i] = groups->lr[i];
    tab.min_lr[i] = groups->min_lr[i];
  }
  PlateauArgs a;
  a.factor = factor; a.threshold = threshold; a.eps = eps;
  a.n_groups = n_groups; a.mode = mode; a.threshold_mode = threshold_mode;
  a.patience = patience; a.cooldown = cooldown; a.epoch = epoch;
  MFM_LAUNCH_TIMED(plateau_step_kernel, dim3(1), dim3(64), 0, stream, state, metric_dev, metric, tab, a);
  MFM_LAUNCH_CHECK("plateau_step_kernel");
  return MFM_OK;
}

}  // namespace mfm

extern "C" int mfm_plateau_step(MfmPlateauState* state, const float* metric_dev, double metric, const MfmPlateauGroups* groups,
                                int32_t n_groups, int32_t mode, int32_t threshold_mode, double factor, double threshold,
                                double eps, int32_t patience, int32_t cooldown, int32_t epoch, void* stream) {
  return mfm::plateau_step_launch(state, metric_dev, metric, groups, n_groups, mode, threshold_mode, factor, threshold, eps,
                                  patience, cooldown, epoch, (hipStream_t)stream);
}
