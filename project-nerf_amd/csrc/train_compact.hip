// The data side of one training step THROUGH the occupancy grid in one launch: what nerf_train_batch_shard
// (sample.hip) followed by nerf_sample_compact_jitter_shard / _chain (compact.hip) compute in two, without the [batch, S] depths
// of the first that the second never reads and without the second's re-read of the rays.  Thread per (ray, sample), as in the
// compaction.  EVERY thread re-forms its ray from the pixel draw and the pose -- two generator draws, one 3x3 rotation, one
// normalisation: about a hundred instructions, no LDS staging, no dependence on another workgroup's stores -- and only the
// thread of sample 0 fetches the pixel and writes rays_o / rays_d / rgba / target.  The pixel ray and the composited target, the
// jittered depth, the voxel test, the slot reservation (wave ballots -> 64 counts in LDS -> one wave scans -> ONE returning atomic
// per workgroup and pass of 4096 samples), the compact-row store and the count hand-off are ray_front.h's, the very functions
// sample.hip and compact.hip call (draw = 1, first_sample = first_ray * n_samples), so every output equals the two-call form's
// bit for bit (the compact rows up to the arbitrary slot order both share).  The compaction normalises the unit direction it
// reads from rays_d a SECOND time; so does the row store here.  Count publication -- plain form: a device word the call clears;
// chain form: two counters used alternately, tickets, (count, seq) in host-mapped memory -- follows compact.hip's protocol, and
// links of both entries alternate on one chain_state.
#include "ray_front.h"

namespace nerf {

struct TrainCompactArgs {
  const float* images;
  const float* poses;
  const float* bg;
  const uint8_t* grid;
  float* rays_o;
  float* rays_d;
  float* rgba;
  float* target;
  float* z_out;
  int* slot_of_sample;
  float* pts_c;
  float* dirs_c;
  unsigned* count;                // the word this call counts in
  unsigned* chain_state;          // chain form: the two counters and the tickets; NULL: plain form
  unsigned* count_host;           // chain form: host-mapped (count, seq) or NULL
  uint64_t key, ray_ctr, sample_ctr;   // generator: key, counter word of ray 0's pixel draw, counter word of sample 0's jitter
  unsigned n_pixels, total, seq;
  int turn, H, W, S, res;
  float half_w, half_h, focal, scene_scale, near_p, far_p, step, bound, scale;
};

__global__ void __launch_bounds__(kCompactThreads) train_batch_compact_kernel(const TrainCompactArgs a) {
  if (a.chain_state != nullptr && blockIdx.x == 0 && threadIdx.x == 0) a.chain_state[a.turn ^ 1] = 0u;  // the NEXT link's counter
  const float* __restrict__ poses = a.poses;
  const uint8_t* __restrict__ grid = a.grid;
  // The argument block alone is ~60 scalar registers, all live across the pass loop: with the generator's 64-bit arithmetic on top
  // the kernel would keep two dozen of them in spill lanes.  What only the thread of sample 0 or only an active sample uses, and
  // the fp32 constants, are held in vector registers instead (128 are there for the taking at 1024 threads; the kernel uses < 110).
  const float* images = a.images;
  const float* bg = a.bg;
  float *rays_o = a.rays_o, *rays_d = a.rays_d, *rgba = a.rgba, *target = a.target, *pts_c = a.pts_c, *dirs_c = a.dirs_c;
  int* slot_of_sample = a.slot_of_sample;
  float half_w = a.half_w, half_h = a.half_h, focal = a.focal, scene_scale = a.scene_scale, near_p = a.near_p, far_p = a.far_p,
        step = a.step, bound = a.bound, scale = a.scale;
  asm volatile("" : "+v"(images), "+v"(bg), "+v"(rays_o), "+v"(rays_d), "+v"(rgba), "+v"(target), "+v"(pts_c), "+v"(dirs_c),
               "+v"(slot_of_sample));
  asm volatile("" : "+v"(half_w), "+v"(half_h), "+v"(focal), "+v"(scene_scale), "+v"(near_p), "+v"(far_p), "+v"(step), "+v"(bound),
               "+v"(scale));
  const unsigned total = a.total;                       // < 2^31: 32-bit sample indices throughout
  const unsigned span = (unsigned)kCompactThreads * kCompactPer;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int S = a.S, res = a.res;
  __shared__ unsigned seg[64];                          // per (k, wave): active count, then first slot
  // uniform trip count so that every lane takes part in the ballots
  for (unsigned g0 = blockIdx.x * span; g0 < total; g0 += gridDim.x * span) {
    float px[kCompactPer], py[kCompactPer], pz[kCompactPer], ux[kCompactPer], uy[kCompactPer], uz[kCompactPer];
    unsigned long long ballot[kCompactPer];
#pragma unroll
    for (int k = 0; k < kCompactPer; ++k) {
      const unsigned g = g0 + (unsigned)k * kCompactThreads + threadIdx.x;
      bool active = false;
      px[k] = py[k] = pz[k] = ux[k] = uy[k] = uz[k] = 0.f;
      if (g < total) {
        const unsigned r = g / (unsigned)S;
        const int s = (int)(g - r * (unsigned)S);
        // ---- the ray (train_batch_kernel + gather_one): one draw over all pixels of all frames, indexed by the GLOBAL ray
        // (counter << 40) + (1 << 39) + 2 * (r + first_ray); n_pixels < 2^32, so the drawn index is divided in 32 bits: the same
        // column, row and frame as train_batch_kernel's 64-bit divisions
        const uint64_t c0 = a.ray_ctr + 2 * (uint64_t)r;
        const uint64_t r64 = ((uint64_t)squares32(c0, a.key) << 32) | squares32(c0 + 1, a.key);
        const unsigned idx = (unsigned)__umul64hi(r64, (uint64_t)a.n_pixels);        // uniform over [0, n_pixels)
        const unsigned row = idx / (unsigned)a.W, frame = row / (unsigned)a.H;
        const int64_t ix = (int64_t)(idx - row * (unsigned)a.W), iy = (int64_t)(row - frame * (unsigned)a.H), im = (int64_t)frame;
        float d[3], o[3];
        pixel_ray(poses + im * 16, ix, iy, half_w, half_h, focal, scene_scale, d, o);
        ux[k] = d[0]; uy[k] = d[1]; uz[k] = d[2];
        if (s == 0) {
          rays_d[(size_t)r * 3 + 0] = ux[k]; rays_d[(size_t)r * 3 + 1] = uy[k]; rays_d[(size_t)r * 3 + 2] = uz[k];
          rays_o[(size_t)r * 3 + 0] = o[0]; rays_o[(size_t)r * 3 + 1] = o[1]; rays_o[(size_t)r * 3 + 2] = o[2];
          const float4 c = *reinterpret_cast<const float4*>(images + ((im * a.H + iy) * a.W + ix) * 4);
          if (rgba != nullptr) *reinterpret_cast<float4*>(rgba + (size_t)r * 4) = c;
          if (target != nullptr) composite_target(target + (size_t)r * 3, c, bg);
        }
        // ---- the sample (sample_compact_kernel, draw = 1): jittered depth from squares_uniform(counter, first_ray * n_samples + g,
        // key), point, voxel test
        const float z = jitter_depth(plain_depth(s, S, step, near_p, far_p), s, S, step, near_p, far_p,
                                     (float)(squares32(a.sample_ctr + (uint64_t)g, a.key) >> 8) * 5.9604644775390625e-08f);
        a.z_out[g] = z;
        px[k] = add_rn(o[0], mul_rn(ux[k], z));
        py[k] = add_rn(o[1], mul_rn(uy[k], z));
        pz[k] = add_rn(o[2], mul_rn(uz[k], z));
        active = voxel_active(grid, res, bound, scale, px[k], py[k], pz[k]);
      }
      ballot[k] = __ballot(active);
      if (lane == 0) seg[k * kCompactWaves + wave] = (unsigned)__popcll(ballot[k]);
    }
    reserve_slots(seg, a.count, lane, wave);
#pragma unroll
    for (int k = 0; k < kCompactPer; ++k) {
      const unsigned g = g0 + (unsigned)k * kCompactThreads + threadIdx.x;
      if (g < total) {
        int slot = -1;
        if ((ballot[k] >> lane) & 1ull) {
          slot = (int)(seg[k * kCompactWaves + wave] + ballot_rank(ballot[k], lane));
          store_compact_row(pts_c, dirs_c, slot, px[k], py[k], pz[k], ux[k], uy[k], uz[k]);
        }
        slot_of_sample[g] = slot;
      }
    }
    __syncthreads();                                    // seg is rewritten by the next pass
  }
  if (a.chain_state != nullptr && a.count_host != nullptr && threadIdx.x == 0)       // chain form
    publish_count(a.chain_state + 2, a.count, a.count_host, a.seq);
}

}  // namespace nerf

using namespace nerf;

// count: the word this call counts in; next_count / tickets / count_host / seq: the chain form's (all NULL / 0 in the plain form,
// which clears `count` with a fill ahead of the launch)
static int train_batch_compact_impl(const char* what, const float* images, const float* poses, int n_images, int H, int W, float focal,
                                    float scene_scale, const float* bg, uint64_t seed, uint64_t counter, int64_t first_ray,
                                    int64_t batch, int n_samples, float near_plane, float far_plane, const uint8_t* binary_grid,
                                    int resolution, float bound, float* rays_o, float* rays_d, float* rgba, float* target,
                                    float* z_out, int* slot_of_sample, float* pts_compact, float* dirs_compact, unsigned* count,
                                    bool chain, int turn, unsigned* count_host, unsigned seq, nerf_stream_t stream) {
  NERF_REQUIRE(batch >= 0, "%s: batch=%lld", what, (long long)batch);
  if (batch == 0) return NERF_OK;
  NERF_REQUIRE(n_samples >= 2, "%s: n_samples=%d (at least 2)", what, n_samples);
  NERF_REQUIRE(batch * (int64_t)n_samples < ((int64_t)1 << 31), "%s: batch * n_samples = %lld must stay below 2^31", what,
               (long long)(batch * (int64_t)n_samples));
  NERF_REQUIRE(counter < ((uint64_t)1 << 24), "%s: counter=%llu (below 2^24)", what, (unsigned long long)counter);
  NERF_REQUIRE(first_ray >= 0 && first_ray < ((int64_t)1 << 38) && (first_ray + batch) * (int64_t)n_samples < ((int64_t)1 << 39),
               "%s: first_ray=%lld ((first_ray + batch) * n_samples must stay below 2^39)", what, (long long)first_ray);
  NERF_REQUIRE(resolution > 0 && resolution <= 32768, "%s: resolution=%d (1..32768)", what, resolution);
  NERF_REQUIRE(bound > 0.0f, "%s: bound must be positive", what);
  NERF_REQUIRE(n_images > 0 && H > 0 && W > 0, "%s: n_images=%d H=%d W=%d", what, n_images, H, W);
  NERF_REQUIRE((uint64_t)n_images * (uint64_t)H * (uint64_t)W < ((uint64_t)1 << 32), "%s: n_images * H * W must stay below 2^32", what);
  NERF_REQUIRE(focal > 0.0f, "%s: focal must be positive", what);
  NERF_REQUIRE((target == nullptr) == (bg == nullptr), "%s: target and bg go together", what);
  NERF_REQUIRE(images != nullptr, "%s: images is NULL", what);
  NERF_REQUIRE(poses != nullptr, "%s: poses is NULL", what);
  NERF_REQUIRE(binary_grid != nullptr, "%s: binary_grid is NULL", what);
  NERF_REQUIRE(rays_o != nullptr, "%s: rays_o is NULL", what);
  NERF_REQUIRE(rays_d != nullptr, "%s: rays_d is NULL", what);
  NERF_REQUIRE(rgba != nullptr || target != nullptr, "%s: rgba and target are both NULL", what);
  NERF_REQUIRE(z_out != nullptr, "%s: z_out is NULL", what);
  NERF_REQUIRE(slot_of_sample != nullptr, "%s: slot_of_sample is NULL", what);
  NERF_REQUIRE(pts_compact != nullptr, "%s: pts_compact is NULL", what);
  NERF_REQUIRE(dirs_compact != nullptr, "%s: dirs_compact is NULL", what);
  NERF_REQUIRE(count != nullptr, "%s: %s is NULL", what, chain ? "chain_state" : "active_count");
  NERF_REQUIRE(!chain || turn == 0 || turn == 1, "%s: turn=%d (0 or 1)", what, turn);
  NERF_REQUIRE((((uintptr_t)images | (uintptr_t)rgba) & 15) == 0, "%s: images / rgba must be 16-byte aligned", what);
  TrainCompactArgs a;
  a.images = images; a.poses = poses; a.bg = bg; a.grid = binary_grid;
  a.rays_o = rays_o; a.rays_d = rays_d; a.rgba = rgba; a.target = target; a.z_out = z_out;
  a.slot_of_sample = slot_of_sample; a.pts_c = pts_compact; a.dirs_c = dirs_compact;
  if (chain) {
    a.count = count + turn; a.chain_state = count; a.turn = turn; a.count_host = count_host; a.seq = seq;
  } else {
    a.count = count; a.chain_state = nullptr; a.turn = 0; a.count_host = nullptr; a.seq = 0;
    if (hipMemsetAsync(count, 0, sizeof(unsigned), as_stream(stream)) != hipSuccess) return fail(NERF_ELAUNCH, "%s: memset failed", what);
  }
  a.n_pixels = (unsigned)((uint64_t)n_images * (uint64_t)H * (uint64_t)W);
  a.key = squares_key(seed);
  a.ray_ctr = (counter << 40) + ((uint64_t)1 << 39) + 2 * (uint64_t)first_ray;
  a.sample_ctr = (counter << 40) + (uint64_t)first_ray * (uint64_t)n_samples;
  a.total = (unsigned)(batch * (int64_t)n_samples);
  a.H = H; a.W = W; a.S = n_samples; a.res = resolution;
  a.half_w = (float)(W * 0.5); a.half_h = (float)(H * 0.5); a.focal = focal; a.scene_scale = scene_scale;
  a.near_p = near_plane; a.far_p = far_plane; a.step = 1.0f / (float)(n_samples - 1);
  a.bound = bound; a.scale = voxel_scale(resolution, bound);
  const int64_t span = (int64_t)kCompactThreads * kCompactPer;
  int64_t blocks = ((int64_t)a.total + span - 1) / span;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(train_batch_compact_kernel, dim3((int)blocks), dim3(kCompactThreads), 0, as_stream(stream), a);
  return check_launch(what);
}

extern "C" int nerf_train_batch_compact(const float* images, const float* poses, int n_images, int H, int W, float focal,
                                        float scene_scale, const float* bg, uint64_t seed, uint64_t counter, int64_t first_ray,
                                        int64_t batch, int n_samples, float near_plane, float far_plane,
                                        const uint8_t* binary_grid, int resolution, float bound, float* rays_o, float* rays_d,
                                        float* rgba, float* target, float* z_out, int* slot_of_sample, float* pts_compact,
                                        float* dirs_compact, unsigned* active_count, nerf_stream_t stream) {
  return train_batch_compact_impl("nerf_train_batch_compact", images, poses, n_images, H, W, focal, scene_scale, bg, seed, counter,
                                  first_ray, batch, n_samples, near_plane, far_plane, binary_grid, resolution, bound, rays_o, rays_d,
                                  rgba, target, z_out, slot_of_sample, pts_compact, dirs_compact, active_count, false, 0, nullptr, 0,
                                  stream);
}

extern "C" int nerf_train_batch_compact_chain(const float* images, const float* poses, int n_images, int H, int W, float focal,
                                              float scene_scale, const float* bg, uint64_t seed, uint64_t counter, int64_t first_ray,
                                              int64_t batch, int n_samples, float near_plane, float far_plane,
                                              const uint8_t* binary_grid, int resolution, float bound, float* rays_o, float* rays_d,
                                              float* rgba, float* target, float* z_out, int* slot_of_sample, float* pts_compact,
                                              float* dirs_compact, unsigned* chain_state, int turn, unsigned* count_host, unsigned seq,
                                              nerf_stream_t stream) {
  return train_batch_compact_impl("nerf_train_batch_compact_chain", images, poses, n_images, H, W, focal, scene_scale, bg, seed,
                                  counter, first_ray, batch, n_samples, near_plane, far_plane, binary_grid, resolution, bound, rays_o,
                                  rays_d, rgba, target, z_out, slot_of_sample, pts_compact, dirs_compact, chain_state, true, turn,
                                  count_host, seq, stream);
}
