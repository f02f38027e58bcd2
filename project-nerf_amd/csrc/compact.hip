// Occupancy-masked sampling with in-kernel compaction.
// Replaces, for the density-grid branch of render_rays (reference src/renderer.py:303-343), the
// chain  sample -> pts -> get_active_mask -> boolean-index gather -> model -> zeros + masked scatter:
// one kernel generates the depths, forms the points, looks them up in the occupancy bitfield and
// appends the ACTIVE samples' (pts, dirs) to compact arrays; `slot_of_sample` records where each
// sample went (-1 = skipped).  The compositing kernels take that map and treat skipped samples as
// sigma = 0, rgb = 0 (exactly what the reference's zero-filled scatter produces), so no dense
// [R*S, 3] tensors are materialised.  Slots are reserved with ONE returning atomic per 1024-thread
// workgroup and pass of 4096 samples (wave ballots -> LDS -> one wave scans the 64 counts): same-address
// atomics serialise in L2 (one per wave: ~16 k per 2 M samples, most of the kernel's time in round 1;
// one per 1024 samples: still 2048 of them, about half of the 38 us the kernel took).  Slot order is
// arbitrary but consistent within a call.
// Depth, voxel test, slot reservation, row store and count hand-off are ray_front.h's, shared with sample.hip and
// train_compact.hip.
#include "ray_front.h"

namespace nerf {

// what the kernels below need of a call to form its samples
struct CompactSampling {
  const float* rays_o;
  const float* rays_d;
  const float* u;                 // [R, S] uniforms, or NULL
  const uint8_t* grid;
  float* z_out;
  uint64_t key, counter, first_sample;
  int S, res, draw;               // draw: the jitter comes from the counter-based generator (common.h) instead of u
  float near_p, far_p, step, bound, scale;
  bool small;                     // fewer than 2^31 samples: 64-bit division is emulated, ~100 instructions
};

__device__ __forceinline__ int64_t ray_of(int64_t g, int S, bool small) {
  return small ? (int64_t)((unsigned)g / (unsigned)S) : g / S;
}

// sample g of the call: its depth (stored to z_out), its point, and whether the point's voxel is occupied
__device__ __forceinline__ bool compact_sample(const CompactSampling& c, int64_t g, float& px, float& py, float& pz) {
  const float* __restrict__ rays_o = c.rays_o;
  const float* __restrict__ rays_d = c.rays_d;
  const int64_t r = ray_of(g, c.S, c.small);
  const int s = (int)(g - r * c.S);
  float z = plain_depth(s, c.S, c.step, c.near_p, c.far_p);
  if (c.u != nullptr || c.draw)
    z = jitter_depth(z, s, c.S, c.step, c.near_p, c.far_p,
                     c.u != nullptr ? c.u[g] : squares_uniform(c.counter, c.first_sample + (uint64_t)g, c.key));
  c.z_out[g] = z;
  px = add_rn(rays_o[r * 3 + 0], mul_rn(rays_d[r * 3 + 0], z));
  py = add_rn(rays_o[r * 3 + 1], mul_rn(rays_d[r * 3 + 1], z));
  pz = add_rn(rays_o[r * 3 + 2], mul_rn(rays_d[r * 3 + 2], z));
  return voxel_active(c.grid, c.res, c.bound, c.scale, px, py, pz);
}

__global__ void __launch_bounds__(kCompactThreads)
sample_compact_kernel(const CompactSampling call, int64_t total, int* __restrict__ slot_of_sample, float* __restrict__ pts_c,
                      float* __restrict__ dirs_c, unsigned* __restrict__ count, unsigned* __restrict__ zero_out,
                      unsigned* __restrict__ tickets, unsigned* __restrict__ count_host, unsigned seq) {
  if (zero_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *zero_out = 0u;      // the NEXT call's counter (chained form)
  // The arguments, the generator's 64-bit constants and the loop bounds fill the scalar file to its last register; the fp32
  // constants live in vector registers instead (59 of the 64 that 8 waves per SIMD would allow), which keeps every scalar out of
  // spill lanes (train_compact.hip does the same, DESIGN 4.21 "Resources").
  CompactSampling c = call;
  asm volatile("" : "+v"(c.near_p), "+v"(c.far_p), "+v"(c.step), "+v"(c.bound), "+v"(c.scale));
  const int64_t span = (int64_t)kCompactThreads * kCompactPer;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ unsigned seg[64];                          // per (k, wave): active count, then first slot
  // uniform trip count so that every lane takes part in the ballots
  for (int64_t g0 = blockIdx.x * span; g0 < total; g0 += (int64_t)gridDim.x * span) {
    float px[kCompactPer], py[kCompactPer], pz[kCompactPer];
    unsigned long long ballot[kCompactPer];
#pragma unroll
    for (int k = 0; k < kCompactPer; ++k) {
      const int64_t g = g0 + (int64_t)k * kCompactThreads + threadIdx.x;
      bool active = false;
      px[k] = py[k] = pz[k] = 0.f;
      if (g < total) active = compact_sample(c, g, px[k], py[k], pz[k]);
      ballot[k] = __ballot(active);
      if (lane == 0) seg[k * kCompactWaves + wave] = (unsigned)__popcll(ballot[k]);
    }
    reserve_slots(seg, count, lane, wave);
#pragma unroll
    for (int k = 0; k < kCompactPer; ++k) {
      const int64_t g = g0 + (int64_t)k * kCompactThreads + threadIdx.x;
      if (g < total) {
        int slot = -1;
        if ((ballot[k] >> lane) & 1ull) {
          slot = (int)(seg[k * kCompactWaves + wave] + ballot_rank(ballot[k], lane));
          const int64_t r = ray_of(g, c.S, c.small);
          const float* __restrict__ rays_d = c.rays_d;
          store_compact_row(pts_c, dirs_c, slot, px[k], py[k], pz[k], rays_d[r * 3 + 0], rays_d[r * 3 + 1], rays_d[r * 3 + 2]);
        }
        slot_of_sample[g] = slot;
      }
    }
    __syncthreads();                                    // seg is rewritten by the next pass
  }
  if (tickets != nullptr && threadIdx.x == 0) publish_count(tickets, count, count_host, seq);      // chained form
}

// ---- ordered form (option "deterministic"): slots in SAMPLE ORDER, whatever the order the workgroups ran in ----
// The single-pass kernel above reserves each pass's slots with a returning atomic: which pass draws which range of the
// compact arrays depends on scheduling, and with it the order in which every later kernel sums over samples (MFMA
// contractions over the sample index, workgroup partials).  Three launches instead: (1) depths, ray points, occupancy
// lookup -> active flag per sample (slot_of_sample: 0 / -1) and the active count of every (pass, k, wave) segment of 64
// samples; (2) one workgroup scans the segment counts in order; (3) slots = segment start + rank inside the wave's
// ballot, points recomputed from the stored depth (the same two rounded operations: the same bits).
__global__ void __launch_bounds__(kCompactThreads)
sample_compact_count_kernel(const CompactSampling c, int64_t total, int* __restrict__ slot_of_sample, unsigned* __restrict__ seg_count) {
  const int64_t span = (int64_t)kCompactThreads * kCompactPer;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t g0 = blockIdx.x * span; g0 < total; g0 += (int64_t)gridDim.x * span) {
    const int64_t pass = g0 / span;
#pragma unroll
    for (int k = 0; k < kCompactPer; ++k) {
      const int64_t g = g0 + (int64_t)k * kCompactThreads + threadIdx.x;
      bool active = false;
      if (g < total) {
        float px, py, pz;
        active = compact_sample(c, g, px, py, pz);
        slot_of_sample[g] = active ? 0 : -1;
      }
      const unsigned long long ballot = __ballot(active);
      if (lane == 0) seg_count[pass * 64 + k * kCompactWaves + wave] = (unsigned)__popcll(ballot);
    }
  }
}

// exclusive scan of n_seg counts in place (one workgroup of 1024; a carried total between rounds); *count = the total
__global__ void __launch_bounds__(1024) sample_compact_scan_kernel(unsigned* __restrict__ seg, int64_t n_seg, unsigned* __restrict__ count) {
  __shared__ unsigned wave_tot[16];
  __shared__ unsigned carry;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int64_t base = 0; base < n_seg; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const unsigned mine = i < n_seg ? seg[i] : 0u;
    unsigned incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned v = __shfl_up(incl, off);
      if (lane >= off) incl += v;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    unsigned before = carry;
    for (int w = 0; w < wave; ++w) before += wave_tot[w];
    if (i < n_seg) seg[i] = before + incl - mine;
    __syncthreads();
    if (threadIdx.x == 1023) carry = before + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = carry;
}

__global__ void __launch_bounds__(kCompactThreads)
sample_compact_place_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, int64_t n_rays, int S,
                            const float* __restrict__ z, int* __restrict__ slot_of_sample, const unsigned* __restrict__ seg_start,
                            float* __restrict__ pts_c, float* __restrict__ dirs_c) {
  const int64_t total = n_rays * (int64_t)S;
  const int64_t span = (int64_t)kCompactThreads * kCompactPer;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool small = total < (int64_t)1 << 31;
  for (int64_t g0 = blockIdx.x * span; g0 < total; g0 += (int64_t)gridDim.x * span) {
    const int64_t pass = g0 / span;
#pragma unroll
    for (int k = 0; k < kCompactPer; ++k) {
      const int64_t g = g0 + (int64_t)k * kCompactThreads + threadIdx.x;
      const bool active = g < total && slot_of_sample[g] == 0;
      const unsigned long long ballot = __ballot(active);
      if (!active) continue;
      const int slot = (int)(seg_start[pass * 64 + k * kCompactWaves + wave] + ballot_rank(ballot, lane));
      const int64_t r = ray_of(g, S, small);
      const float zz = z[g];
      const float dx = rays_d[r * 3 + 0], dy = rays_d[r * 3 + 1], dz = rays_d[r * 3 + 2];
      store_compact_row(pts_c, dirs_c, slot, add_rn(rays_o[r * 3 + 0], mul_rn(dx, zz)), add_rn(rays_o[r * 3 + 1], mul_rn(dy, zz)),
                        add_rn(rays_o[r * 3 + 2], mul_rn(dz, zz)), dx, dy, dz);
      slot_of_sample[g] = slot;
    }
  }
}

}  // namespace nerf

using namespace nerf;

static int sample_compact_impl(const float* rays_o, const float* rays_d, const float* u, int64_t n_rays,
                               int n_samples, float near_plane, float far_plane, const uint8_t* binary_grid,
                               int resolution, float bound, float* z_out, int* slot_of_sample, float* pts_compact,
                               float* dirs_compact, unsigned* active_count, nerf_stream_t stream,
                               uint64_t key, uint64_t counter, int draw, uint64_t first_sample = 0, void* scratch = nullptr,
                               size_t scratch_bytes = 0, unsigned* next_count = nullptr, unsigned* tickets = nullptr,
                               unsigned* count_host = nullptr, unsigned seq = 0) {
  NERF_REQUIRE(n_rays >= 0 && n_samples >= 2 && resolution > 0 && resolution <= 32768 && bound > 0.0f, "nerf_sample_compact: bad sizes");
  NERF_REQUIRE(active_count != nullptr, "nerf_sample_compact: active_count is NULL");
  // chained form (next_count): active_count was cleared by the previous call of the chain (or by the caller), this call's kernel
  // clears *next_count -- no fill launch per call
  if (next_count == nullptr && hipMemsetAsync(active_count, 0, sizeof(unsigned), as_stream(stream)) != hipSuccess)
    return fail(NERF_ELAUNCH, "nerf_sample_compact: memset failed");
  if (n_rays == 0 && tickets == nullptr) {
    if (next_count != nullptr && hipMemsetAsync(next_count, 0, sizeof(unsigned), as_stream(stream)) != hipSuccess)
      return fail(NERF_ELAUNCH, "nerf_sample_compact: memset failed");
    return NERF_OK;
  }                                                    // (publishing form with no rays: one workgroup that publishes a count of zero)
  NERF_REQUIRE(n_rays == 0 || (rays_o && rays_d && binary_grid && z_out && slot_of_sample && pts_compact && dirs_compact),
               "nerf_sample_compact: NULL pointer");
  const int64_t total = n_rays * (int64_t)n_samples;
  const CompactSampling c{rays_o, rays_d, u, binary_grid, z_out, key, counter, first_sample, n_samples, resolution, draw,
                          near_plane, far_plane, 1.0f / (float)(n_samples - 1), bound, voxel_scale(resolution, bound),
                          total < (int64_t)1 << 31};
  const int64_t span = (int64_t)kCompactThreads * kCompactPer;
  int64_t blocks = (total + span - 1) / span;
  const int64_t n_seg = blocks * 64;                     // before the cap: one (k, wave) segment per 64 samples of every pass
  if (blocks > 1024) blocks = 1024;
  if (blocks < 1) blocks = 1;
  if (scratch != nullptr) {                              // ordered form: slots in sample order
    NERF_REQUIRE(scratch_bytes >= (size_t)n_seg * sizeof(unsigned) && ((uintptr_t)scratch & 3) == 0,
                 "nerf_sample_compact_ordered: scratch of %zu bytes, %zu needed", scratch_bytes, (size_t)n_seg * sizeof(unsigned));
    unsigned* seg = static_cast<unsigned*>(scratch);
    hipLaunchKernelGGL(sample_compact_count_kernel, dim3((int)blocks), dim3(kCompactThreads), 0, as_stream(stream), c, total, slot_of_sample,
                       seg);
    hipLaunchKernelGGL(sample_compact_scan_kernel, dim3(1), dim3(1024), 0, as_stream(stream), seg, n_seg, active_count);
    hipLaunchKernelGGL(sample_compact_place_kernel, dim3((int)blocks), dim3(kCompactThreads), 0, as_stream(stream), rays_o, rays_d, n_rays,
                       n_samples, z_out, slot_of_sample, seg, pts_compact, dirs_compact);
    return check_launch("nerf_sample_compact_ordered");
  }
  hipLaunchKernelGGL(sample_compact_kernel, dim3((int)blocks), dim3(kCompactThreads), 0, as_stream(stream), c, total, slot_of_sample,
                     pts_compact, dirs_compact, active_count, next_count, tickets, count_host, seq);
  return check_launch("nerf_sample_compact");
}

extern "C" int nerf_sample_compact(const float* rays_o, const float* rays_d, const float* u, int64_t n_rays,
                                   int n_samples, float near_plane, float far_plane, const uint8_t* binary_grid,
                                   int resolution, float bound, float* z_out, int* slot_of_sample, float* pts_compact,
                                   float* dirs_compact, unsigned* active_count, nerf_stream_t stream) {
  return sample_compact_impl(rays_o, rays_d, u, n_rays, n_samples, near_plane, far_plane, binary_grid, resolution, bound, z_out,
                             slot_of_sample, pts_compact, dirs_compact, active_count, stream, 0, 0, 0);
}

extern "C" int nerf_sample_compact_jitter_shard(const float* rays_o, const float* rays_d, uint64_t seed, uint64_t counter,
                                                int64_t first_ray, int64_t n_rays, int n_samples, float near_plane, float far_plane,
                                                const uint8_t* binary_grid, int resolution, float bound, float* z_out,
                                                int* slot_of_sample, float* pts_compact, float* dirs_compact,
                                                unsigned* active_count, nerf_stream_t stream) {
  NERF_REQUIRE(first_ray >= 0 && counter < ((uint64_t)1 << 24) && (first_ray + n_rays) * (int64_t)n_samples < ((int64_t)1 << 40),
               "nerf_sample_compact_jitter: counter / batch out of range");
  return sample_compact_impl(rays_o, rays_d, nullptr, n_rays, n_samples, near_plane, far_plane, binary_grid, resolution, bound,
                             z_out, slot_of_sample, pts_compact, dirs_compact, active_count, stream, squares_key(seed), counter, 1,
                             (uint64_t)first_ray * (uint64_t)n_samples);
}

// The same call as a link of a CHAIN of calls on one stream.  chain_state: NERF_COMPACT_CHAIN_WORDS device words, zeroed ONCE by the
// caller: two counters used alternately (this call counts in word `turn` and its kernel clears word `turn ^ 1` for the next link: no
// fill launch per call) and the tickets of the workgroup that finishes last, which writes the count to count_host[0] and then
// `seq` to count_host[1] (host-mapped pinned memory; NULL: no publication): no copy launch, no event -- the host polls for its seq.
extern "C" int nerf_sample_compact_jitter_chain(const float* rays_o, const float* rays_d, uint64_t seed, uint64_t counter,
                                                int64_t first_ray, int64_t n_rays, int n_samples, float near_plane, float far_plane,
                                                const uint8_t* binary_grid, int resolution, float bound, float* z_out,
                                                int* slot_of_sample, float* pts_compact, float* dirs_compact,
                                                unsigned* chain_state, int turn, unsigned* count_host, unsigned seq, nerf_stream_t stream) {
  NERF_REQUIRE(first_ray >= 0 && counter < ((uint64_t)1 << 24) && (first_ray + n_rays) * (int64_t)n_samples < ((int64_t)1 << 40),
               "nerf_sample_compact_jitter_chain: counter / batch out of range");
  NERF_REQUIRE(chain_state != nullptr && (turn == 0 || turn == 1), "nerf_sample_compact_jitter_chain: chain_state NULL or turn not 0 / 1");
  return sample_compact_impl(rays_o, rays_d, nullptr, n_rays, n_samples, near_plane, far_plane, binary_grid, resolution, bound,
                             z_out, slot_of_sample, pts_compact, dirs_compact, chain_state + turn, stream, squares_key(seed), counter, 1,
                             (uint64_t)first_ray * (uint64_t)n_samples, nullptr, 0, chain_state + (turn ^ 1),
                             count_host != nullptr ? chain_state + 2 : nullptr, count_host, seq);
}

extern "C" int nerf_sample_compact_jitter(const float* rays_o, const float* rays_d, uint64_t seed, uint64_t counter,
                                          int64_t n_rays, int n_samples, float near_plane, float far_plane,
                                          const uint8_t* binary_grid, int resolution, float bound, float* z_out,
                                          int* slot_of_sample, float* pts_compact, float* dirs_compact,
                                          unsigned* active_count, nerf_stream_t stream) {
  return nerf_sample_compact_jitter_shard(rays_o, rays_d, seed, counter, 0, n_rays, n_samples, near_plane, far_plane, binary_grid,
                                          resolution, bound, z_out, slot_of_sample, pts_compact, dirs_compact, active_count, stream);
}

extern "C" size_t nerf_sample_compact_ordered_scratch_bytes(int64_t n_rays, int n_samples) {
  if (n_rays <= 0 || n_samples <= 0) return 0;
  const int64_t span = (int64_t)kCompactThreads * kCompactPer;
  return (size_t)((n_rays * n_samples + span - 1) / span) * 64 * sizeof(unsigned);
}

extern "C" int nerf_sample_compact_ordered(const float* rays_o, const float* rays_d, const float* u, int draw, uint64_t seed, uint64_t counter,
                                           int64_t first_ray, int64_t n_rays, int n_samples, float near_plane, float far_plane,
                                           const uint8_t* binary_grid, int resolution, float bound, float* z_out, int* slot_of_sample,
                                           float* pts_compact, float* dirs_compact, unsigned* active_count, void* scratch,
                                           size_t scratch_bytes, nerf_stream_t stream) {
  NERF_REQUIRE(first_ray >= 0 && counter < ((uint64_t)1 << 24) && (first_ray + n_rays) * (int64_t)n_samples < ((int64_t)1 << 40),
               "nerf_sample_compact_ordered: counter / batch out of range");
  NERF_REQUIRE(n_rays == 0 || scratch != nullptr, "nerf_sample_compact_ordered: scratch is NULL");
  return sample_compact_impl(rays_o, rays_d, u, n_rays, n_samples, near_plane, far_plane, binary_grid, resolution, bound, z_out,
                             slot_of_sample, pts_compact, dirs_compact, active_count, stream, squares_key(seed), counter,
                             (u == nullptr && draw) ? 1 : 0, (uint64_t)first_ray * (uint64_t)n_samples, scratch, scratch_bytes);
}
