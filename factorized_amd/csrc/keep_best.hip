// "Keep the best weights" on one flat parameter buffer (factorized_amd.checkpoint.KeepBest; the reference's
// `if valid_loss <= best_valid: best_valid = valid_loss; torch.save(model, ...)`, mfm_mosi.py:467-481): ONE launch compares a
// metric with the best value so far and, if it is at least as good, copies the range [begin, end) of the live parameters `p`
// into the snapshot `best` of the same layout.  Comparison, copy and bookkeeping all happen on the device, so the metric never
// has to reach the host and a captured launch takes its decision anew on every replay.
//
// The state block (MfmKeepBestState, include/mfm_hip.h) lives in device memory: best_value, calls (launches so far), best_call
// (0-based index of the launch that last took a snapshot, -1: none), taken (1: the latest launch took one) and a ticket word
// that is 0 between launches.  The metric is one device float (`metric_dev`), or, when that pointer is null, the float kernel
// argument `metric_host`.  Every wave reads best_value, calls and the metric before anything else and decides
//     take = metric <= best_value  (MFM_KEEP_MIN)     take = metric >= best_value  (MFM_KEEP_MAX)
// -- the reference's `<=`: a tie takes the newer weights, a NaN metric compares false and never takes.  take is uniform over
// the launch.  Not taken: no parameter byte is loaded or stored.  Taken: the tiles are copied bit for bit, no arithmetic touches
// them (NaN payloads and -0.0 survive).  Behind its last tile a workgroup draws an arrival ticket (one agent-scope fetch_add,
// acquire-release); the workgroup that draws gridDim.x - 1 stores the new state from one lane -- best_value = metric and
// best_call = calls when taken, taken, calls + 1 -- and only then puts the ticket word back to 0.  Nobody waits or spins: this
// is a ticket, not a barrier, and a 1-workgroup launch takes the same code.
//
// Why no workgroup can see the new best_value (or calls) too early.  The state is stored by ONE lane, the one whose fetch_add
// returned gridDim.x - 1, i.e. after every workgroup's lane 0 has drawn.  In a workgroup, (1) every wave branches on `take`
// before its first tile, with or without a tile of its own, so its loads of best_value, calls and the metric have returned
// before it reaches the __syncthreads() (the generated code waits vmcnt(0) in front of the compare); (2) lane 0 draws behind
// that __syncthreads(), and the release half of its fetch_add keeps its own loads in front of the draw; (3) the acquire half
// of the last arriver's fetch_add keeps its stores of the state behind every earlier draw in the ticket word's modification
// order.  So each load of the old state happens before its workgroup's draw, every draw happens before the last one, and the
// last one happens before the stores.  The ticket's 0 is stored last, by the same lane, and the next launch on the stream
// starts behind the end of this one: it finds 0.  One launch at a time may use a state block.
//
// Work is dealt as in the other flat kernels (span_tiles.h, avg.hip): 256 threads, one float4 per thread and tile, at most
// 2048 workgroups grid-striding over the tiles, 128-bit loads and stores, no LDS.  8 bytes of traffic per element when
// taken, none when not.
//
// Compiler resource report (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage):
//   keep_best_flat_kernel   VGPRs 12   AGPRs 0   SGPRs 24  scratch 0 bytes   LDS 0 bytes   occupancy 8 waves/SIMD
// In the generated code every wave waits for its loads of the state and the metric (s_waitcnt vmcnt(0)) before the compare
// and the branch, the tiles move as global_load_dwordx4 / global_store_dwordx4, and the four state words and the ticket's 0
// leave as vector stores (global_store_dword ... sc1) from one lane.
#include "span_tiles.h"

namespace mfm {

#define KB_LOAD(ptr) __hip_atomic_load(ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define KB_STORE(ptr, v) __hip_atomic_store(ptr, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

__global__ __launch_bounds__(kSpanTile) void keep_best_flat_kernel(float* best, const float* p, int64_t b4, int64_t e4, int tiles,
                                                                   int mode, const float* metric_dev, float metric_host,
                                                                   MfmKeepBestState* st) {
  const float best_value = KB_LOAD(&st->best_value);
  const int32_t calls = KB_LOAD(&st->calls);
  const float metric = metric_dev ? KB_LOAD(metric_dev) : metric_host;
  const bool take = mode == MFM_KEEP_MIN ? metric <= best_value : metric >= best_value;      // (false for a NaN on either side)
  if (take) {
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
      const int64_t i = b4 + (int64_t)t * kSpanTile + threadIdx.x;
      if (i >= e4) continue;
      reinterpret_cast<f32x4*>(best)[i] = reinterpret_cast<const f32x4*>(p)[i];          // bit for bit
    }
  }
  __syncthreads();          // every wave of this workgroup is past its loads of the state and the metric
  if (threadIdx.x == 0) {
    const int drawn = __hip_atomic_fetch_add(&st->ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (drawn == (int)gridDim.x - 1) {
      if (take) {
        KB_STORE(&st->best_value, metric);
        KB_STORE(&st->best_call, calls);
      }
      KB_STORE(&st->taken, take ? 1 : 0);
      KB_STORE(&st->calls, calls + 1);
      KB_STORE(&st->ticket, 0);
    }
  }
}

int keep_best_flat_launch(float* best, const float* p, int64_t begin, int64_t end, int mode, const float* metric_dev,
                          float metric, MfmKeepBestState* state, hipStream_t stream) {
  static const char* who = "keep best flat";
  MFM_REQUIRE(best && p && state, "%s: bad arguments (best, p and state must not be null)", who);
  MFM_REQUIRE((((uintptr_t)best | (uintptr_t)p) & 15) == 0, "%s: best and p must be 16-byte aligned", who);
  MFM_REQUIRE(begin >= 0 && end > begin && (begin & 3) == 0 && (end & 3) == 0,
              "%s: [%lld,%lld) (bounds multiples of 4 elements, end above begin)", who, (long long)begin, (long long)end);
  MFM_REQUIRE(mode == MFM_KEEP_MIN || mode == MFM_KEEP_MAX, "%s: unknown mode %d", who, mode);
  MFM_REQUIRE(((uintptr_t)state & 15) == 0 && ((uintptr_t)metric_dev & 3) == 0,
              "%s: state must be 16-byte aligned (an MfmKeepBestState) and the device metric 4-byte aligned", who);
  const int64_t b4 = begin >> 2, e4 = end >> 2;
  int32_t tiles;
  int nb;
  if (int rc = span_grid(who, (e4 - b4 + kSpanTile - 1) / kSpanTile, &tiles, &nb)) return rc;
  MFM_LAUNCH_TIMED(keep_best_flat_kernel, dim3(nb), dim3(kSpanTile), 0, stream, best, p, b4, e4, (int)tiles, mode, metric_dev,
                   metric, state);
  MFM_LAUNCH_CHECK("keep_best_flat_kernel");
  return MFM_OK;
}

}  // namespace mfm

extern "C" int mfm_keep_best_flat(float* best, const float* p, int64_t begin, int64_t end, int32_t mode, const float* metric_dev,
                                  float metric, MfmKeepBestState* state, void* stream) {
  return mfm::keep_best_flat_launch(best, p, begin, end, mode, metric_dev, metric, state, (hipStream_t)stream);
}
