// The ray front end, each piece ONCE: stratified depth, voxel test, slot reservation, compact-row store, count
// hand-off, pixel ray and composited target.  Included by sample.hip (dense sampling, ray gather, train_batch), compact.hip
// (occupancy-masked sampling with compaction) and train_compact.hip (both in one launch).  The tests hold those three files to
// each other bit for bit and links of compact.hip's and train_compact.hip's chain entries alternate on one chain_state, so a
// change here is a change to all three.  Every fp32 step is mul_rn / add_rn / sub_rn, an explicit __builtin_fmaf, a division
// or a sqrtf: nothing here can be contracted, whatever -ffp-contract the including file is built with.
#pragma once
#include "common.h"

namespace nerf {

// ---- stratified depth (reference src/renderer.py:186-201) ----
// torch.linspace(0,1,S) on CPU: step = 1/(S-1) in fp32; the lower half walks up
// from 0, the upper half walks down from 1, each with ONE rounding.
__device__ __forceinline__ float linspace01(int i, int n, float step) {
  if (i < n / 2) return mul_rn(step, (float)i);
  return __builtin_fmaf(-step, (float)(n - 1 - i), 1.0f);
}

__device__ __forceinline__ float plain_depth(int i, int n, float step, float near_p, float far_p) {
  const float t = linspace01(i, n, step);
  // near*(1-t) + far*t, three roundings (src/renderer.py:190)
  return add_rn(mul_rn(near_p, sub_rn(1.0f, t)), mul_rn(far_p, t));
}

// jittered depth of sample i given its plain depth zi and its uniform draw u (src/renderer.py:195-199: mids / upper / lower).
// zi is an argument because the callers compute it anyway: computed here a second time, the branch of linspace01 would be
// taken twice per sample (the compiler does not merge the two).
__device__ __forceinline__ float jitter_depth(float zi, int i, int n, float step, float near_p, float far_p, float u) {
  float lo = zi, hi = zi;
  if (i > 0) lo = mul_rn(0.5f, add_rn(zi, plain_depth(i - 1, n, step, near_p, far_p)));
  if (i < n - 1) hi = mul_rn(0.5f, add_rn(plain_depth(i + 1, n, step, near_p, far_p), zi));
  return add_rn(lo, mul_rn(sub_rn(hi, lo), u));
}

// ---- voxel test of a point against the res^3 occupancy bitfield (src/renderer.py:145) ----
// the Python double res/(2*bound) is demoted to fp32 before the multiply
inline float voxel_scale(int res, float bound) { return (float)((double)res / (2.0 * (double)bound)); }

// (p + bound) * scale, then .long(), which truncates toward zero: (-1, res) is exactly the range of values whose index lands in [0, res)
__device__ __forceinline__ bool voxel_active(const uint8_t* __restrict__ grid, int res, float bound, float scale, float px, float py,
                                             float pz) {
  const float fx = mul_rn(add_rn(px, bound), scale), fy = mul_rn(add_rn(py, bound), scale), fz = mul_rn(add_rn(pz, bound), scale),
              fres = (float)res;
  if (fx > -1.0f && fx < fres && fy > -1.0f && fy < fres && fz > -1.0f && fz < fres)
    return grid[((int64_t)((int)fx * res + (int)fy)) * res + (int)fz] != 0;
  return false;
}

// ---- slot reservation: 1024 threads, 4 samples per thread and pass, ONE returning atomic per workgroup and pass of 4096 samples ----
constexpr int kCompactThreads = 1024;
constexpr int kCompactPer = 4;                          // samples per thread and pass: 4096 samples share one atomic
constexpr int kCompactWaves = kCompactThreads / 64;
static_assert(kCompactPer * kCompactWaves == 64, "the (k, wave) counts of a pass are scanned by one wave");

// seg[k * kCompactWaves + wave] holds the active count of every (k, wave) ballot of the pass on entry and the first slot of that
// segment on return.  Every thread of the workgroup calls it (two barriers); the caller puts one more barrier before it rewrites seg.
__device__ __forceinline__ void reserve_slots(unsigned* seg, unsigned* count, int lane, int wave) {
  __syncthreads();
  if (wave == 0) {                                      // exclusive scan of the 64 counts; ONE returning atomic per pass
    const unsigned mine = seg[lane];
    unsigned incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned v = __shfl_up(incl, off);
      if (lane >= off) incl += v;
    }
    unsigned base = 0;
    if (lane == 63 && incl != 0) base = atomicAdd(count, incl);
    base = __shfl(base, 63);
    seg[lane] = base + incl - mine;
  }
  __syncthreads();
}

// rank of an active lane among the active lanes of its wave's ballot
__device__ __forceinline__ unsigned ballot_rank(unsigned long long ballot, int lane) {
  return (unsigned)__popcll(ballot & ((1ull << lane) - 1ull));
}

// ---- compact row `slot`: the point, and the ray direction normalised (again: the callers' directions are unit already) ----
// slot < the number of samples (the active count never exceeds it): inside the capacity of pts_c / dirs_c
__device__ __forceinline__ void store_compact_row(float* __restrict__ pts_c, float* __restrict__ dirs_c, int slot, float px, float py,
                                                  float pz, float dx, float dy, float dz) {
  const float nrm = sqrtf(add_rn(add_rn(mul_rn(dx, dx), mul_rn(dy, dy)), mul_rn(dz, dz)));
  pts_c[(size_t)slot * 3 + 0] = px; pts_c[(size_t)slot * 3 + 1] = py; pts_c[(size_t)slot * 3 + 2] = pz;
  dirs_c[(size_t)slot * 3 + 0] = dx / nrm; dirs_c[(size_t)slot * 3 + 1] = dy / nrm; dirs_c[(size_t)slot * 3 + 2] = dz / nrm;
}

// ---- count hand-off of the chained form ----
// The workgroup that finishes last hands the count to the host -- two words of host-mapped pinned memory, the call's sequence
// number written last behind a system-scope fence -- instead of a copy launch and an event behind the kernel (each of those
// packets cost the stream a ~5-us gap of its own).  Tickets in two stages (32 groups: same-address atomics retire serially);
// every ticket word is back at zero when the last workgroup has passed.  Called by ONE thread per workgroup, the one whose
// returning atomics on *count were the workgroup's last (they have returned: their values were used), once its passes are over.
__device__ __forceinline__ void publish_count(unsigned* tickets, unsigned* count, unsigned* count_host, unsigned seq) {
  const unsigned B = gridDim.x, g = blockIdx.x % 32u, in_group = (B - g + 31u) / 32u;
  if (atomicAdd(&tickets[1 + g], 1u) == in_group - 1) {
    atomicExch(&tickets[1 + g], 0u);
    if (atomicAdd(&tickets[0], 1u) == (B < 32u ? B : 32u) - 1) {
      atomicExch(&tickets[0], 0u);
      volatile unsigned* host = count_host;
      host[0] = atomicOr(count, 0u);
      __threadfence_system();
      host[1] = seq;
    }
  }
}

// ---- pixel ray (reference src/dataset.py:150-171) ----
// camera-space direction of pixel (px, py) (no +0.5 centre offset, -y, -z), rotation by c2w[:3,:3] with every product and sum
// rounded on its own, normalisation; origin = c2w[:3,3], scaled only when scene_scale != 1
__device__ __forceinline__ void pixel_ray(const float* __restrict__ c2w, int64_t px, int64_t py, float half_w, float half_h, float focal,
                                          float scene_scale, float d[3], float o[3]) {
  const float x = sub_rn((float)px, half_w) / focal;
  const float y = -(sub_rn((float)py, half_h) / focal);
  const float z = -1.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    d[i] = add_rn(add_rn(mul_rn(c2w[4 * i + 0], x), mul_rn(c2w[4 * i + 1], y)), mul_rn(c2w[4 * i + 2], z));
    const float t = c2w[4 * i + 3];
    o[i] = scene_scale != 1.0f ? mul_rn(t, scene_scale) : t;
  }
  const float nrm = sqrtf(add_rn(add_rn(mul_rn(d[0], d[0]), mul_rn(d[1], d[1])), mul_rn(d[2], d[2])));
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = d[i] / nrm;
}

// target = rgb * a + bg * (1 - a), every product and sum rounded on its own (run.py:317-322)
__device__ __forceinline__ void composite_target(float* __restrict__ target, float4 c, const float* __restrict__ bg) {
  const float rest = sub_rn(1.0f, c.w);
  target[0] = add_rn(mul_rn(c.x, c.w), mul_rn(bg[0], rest));
  target[1] = add_rn(mul_rn(c.y, c.w), mul_rn(bg[1], rest));
  target[2] = add_rn(mul_rn(c.z, c.w), mul_rn(bg[2], rest));
}

}  // namespace nerf
