// The counted render chain, shared by the two evaluation entries that go through an occupancy grid (render_grid.hip: the vanilla
// 8x256 field; render_instant.hip: the Instant-NGP field).  render_rays without perturbation against a density_grid for ANY number
// of rays as one launch chain (reference render_rays' masked branch, src/renderer.py:303-343 of 240-384; render_image's chunk loop,
// 387-418; the field query, src/core.py:354-359).  Per chunk of `chunk_rays` rays, all on the caller's stream:
//   clear the count word -> nerf_sample_compact (plain depths) -> the entry's field launches -> nerf_composite_fwd_indexed.
// The compaction leaves the active count in a DEVICE word; the field launches behind it read it there (the *_counted forms of
// common.h) and are sized for the chunk's capacity, so no host ever reads the count: no allocation, no host synchronisation,
// graph-capturable, ONE caller-provided workspace.  A skipped sample contributes sigma = 0 and rgb = 0; a chunk without an active
// sample renders the background, depth 0, acc 0 -- the reference's forced query of sample 0 of the first ray
// (src/renderer.py:309-311) keeps an autograd graph connected and is not reproduced here.
// Host code only.  Every refusal begins with `what`, the name of the entry that was called.
#pragma once
#include "common.h"

namespace nerf {

// byte offsets into the workspace; the count word sits at offset 0
struct CountedRenderLayout { size_t z, slots, pts, dirs, image, rgb, sigma, total; };

// image_row_bytes: bytes per sample of the operand image between the compaction and the decoder, its rows padded to a multiple
// of 128 samples (0: the entry has none, and the piece takes no room)
inline CountedRenderLayout counted_render_layout(int64_t chunk_rays, int n_samples, size_t image_row_bytes) {
  const size_t n = (size_t)chunk_rays * (size_t)n_samples, n_pad = (n + 127) / 128 * 128;
  CountedRenderLayout l{};
  size_t o = 256;                          // header: the active count
  l.z = piece(&o, n * 4);
  l.slots = piece(&o, n * 4);
  l.pts = piece(&o, n * 12);
  l.dirs = piece(&o, n * 12);
  l.image = piece(&o, n_pad * image_row_bytes);
  l.rgb = piece(&o, n * 12);
  l.sigma = piece(&o, n * 4);
  l.total = o;
  return l;
}

inline size_t counted_render_workspace_bytes(int64_t chunk_rays, int n_samples, size_t image_row_bytes) {
  if (chunk_rays <= 0 || n_samples <= 0) return 0;
  return counted_render_layout(chunk_rays, n_samples, image_row_bytes).total;
}

// the checks both entries make of their common arguments (the entry has made its own and has returned for n_rays <= 0)
inline int counted_render_check(const char* what, const uint8_t* binary_grid, int grid_resolution, float grid_bound, const float* rays_o,
                                const float* rays_d, int64_t n_rays, int n_samples, const float* bg, int64_t bg_rows,
                                int64_t chunk_rays, const void* workspace, const float* out_rgb, const float* out_depth,
                                const float* out_acc) {
  NERF_REQUIRE(n_samples >= 2 && n_samples <= 1024 && chunk_rays > 0, "%s: n_samples=%d (2..1024) chunk=%lld", what, n_samples,
               (long long)chunk_rays);
  NERF_REQUIRE(chunk_rays < ((int64_t)1 << 31) && chunk_rays * (int64_t)n_samples < ((int64_t)1 << 31),
               "%s: chunk too large (chunk_rays * n_samples must stay below 2^31)", what);
  NERF_REQUIRE(grid_resolution > 0 && grid_resolution <= 32768 && grid_bound > 0.0f,
               "%s: grid_resolution=%d (1..32768), grid_bound must be positive", what, grid_resolution);
  NERF_REQUIRE(bg == nullptr || bg_rows == 1 || bg_rows == n_rays, "%s: bg_rows=%lld", what, (long long)bg_rows);
  NERF_REQUIRE(binary_grid && rays_o && rays_d && workspace && out_rgb && out_depth && out_acc, "%s: NULL pointer", what);
  NERF_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", what);
  return NERF_OK;
}

// field(pts, dirs, count, capacity, image, rgb, sigma) queues the entry's launches for the rows [0, *count) of pts / dirs (image:
// the operand-image piece of the workspace) and returns their status
template <class Field>
int counted_render(const char* what, size_t image_row_bytes, const uint8_t* binary_grid, int grid_resolution, float grid_bound,
                   const float* rays_o, const float* rays_d, int64_t n_rays, int n_samples, float near_plane, float far_plane,
                   const float* bg, int64_t bg_rows, int64_t chunk_rays, void* workspace, float* out_rgb, float* out_depth,
                   float* out_acc, nerf_stream_t stream, Field field) {
  const int ok = counted_render_check(what, binary_grid, grid_resolution, grid_bound, rays_o, rays_d, n_rays, n_samples, bg, bg_rows,
                                      chunk_rays, workspace, out_rgb, out_depth, out_acc);
  if (ok != NERF_OK) return ok;
  const CountedRenderLayout l = counted_render_layout(chunk_rays, n_samples, image_row_bytes);
  char* w = static_cast<char*>(workspace);
  unsigned* count = reinterpret_cast<unsigned*>(w);
  float* z = reinterpret_cast<float*>(w + l.z);
  int* slots = reinterpret_cast<int*>(w + l.slots);
  float* pts = reinterpret_cast<float*>(w + l.pts);
  float* dirs = reinterpret_cast<float*>(w + l.dirs);
  float* rgb = reinterpret_cast<float*>(w + l.rgb);
  float* sigma = reinterpret_cast<float*>(w + l.sigma);
  const int64_t capacity = chunk_rays * (int64_t)n_samples;       // sizes the counted launches of EVERY chunk (the last may hold fewer rays)
  for (int64_t r0 = 0; r0 < n_rays; r0 += chunk_rays) {
    const int64_t r = n_rays - r0 < chunk_rays ? n_rays - r0 : chunk_rays;
    // (nerf_sample_compact clears the count word on the stream before its kernel adds to it)
    int rc = nerf_sample_compact(rays_o + r0 * 3, rays_d + r0 * 3, nullptr, r, n_samples, near_plane, far_plane, binary_grid, grid_resolution,
                                 grid_bound, z, slots, pts, dirs, count, stream);
    if (rc != NERF_OK) return rc;
    rc = field(pts, dirs, count, capacity, w + l.image, rgb, sigma);
    if (rc != NERF_OK) return rc;
    rc = nerf_composite_fwd_indexed(rgb, sigma, slots, z, rays_d + r0 * 3, bg == nullptr ? nullptr : (bg_rows > 1 ? bg + r0 * 3 : bg),
                                    bg_rows > 1 ? r : bg_rows, r, n_samples, out_rgb + r0 * 3, out_depth + r0, out_acc + r0, stream);
    if (rc != NERF_OK) return rc;
  }
  return NERF_OK;
}

}  // namespace nerf
