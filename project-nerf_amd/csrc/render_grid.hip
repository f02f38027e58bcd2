// Evaluation entry of the vanilla (8x256) field through an occupancy grid: render_rays without perturbation against a density_grid
// for ANY number of rays as one launch chain (reference render_rays' masked branch, src/renderer.py:303-343 of 240-384;
// render_image's chunk loop, 387-418; the field query, src/core.py:354-359).  Per chunk of `chunk_rays` rays, all on the caller's stream:
//   clear the count word -> nerf_sample_compact (plain depths) -> the inference chain in point mode -> nerf_composite_fwd_indexed.
// The compaction leaves the active count in a DEVICE word; the decoder launch behind it reads it there (mlp_fwd_counted: common.h)
// and is sized for the chunk's capacity, so no host ever reads the count: no allocation, no host synchronisation, graph-capturable,
// ONE caller-provided workspace.  A skipped sample contributes sigma = 0 and rgb = 0; a chunk without an active sample renders the
// background, depth 0, acc 0 -- the reference's forced query of sample 0 of the first ray (src/renderer.py:309-311) keeps an
// autograd graph connected and is not reproduced here.
#include "common.h"

namespace {

struct GridRenderLayout { size_t z, slots, pts, dirs, rgb, sigma, total; };   // the count word sits at offset 0

size_t piece(size_t* o, size_t bytes) {
  const size_t at = *o;
  *o += (bytes + 255) / 256 * 256;
  return at;
}

GridRenderLayout grid_render_layout(int64_t chunk_rays, int n_samples) {
  const size_t n = (size_t)chunk_rays * (size_t)n_samples;
  GridRenderLayout l{};
  size_t o = 256;                          // header: the active count
  l.z = piece(&o, n * 4);
  l.slots = piece(&o, n * 4);
  l.pts = piece(&o, n * 12);
  l.dirs = piece(&o, n * 12);
  l.rgb = piece(&o, n * 12);
  l.sigma = piece(&o, n * 4);
  l.total = o;
  return l;
}

}  // namespace

extern "C" size_t nerf_render_rays_grid_workspace_bytes(int64_t chunk_rays, int n_samples) {
  if (chunk_rays <= 0 || n_samples <= 0) return 0;
  return grid_render_layout(chunk_rays, n_samples).total;
}

extern "C" int nerf_render_rays_grid_fwd(const void* packed, const uint8_t* binary_grid, int grid_resolution, float grid_bound,
                                         const float* rays_o, const float* rays_d, int64_t n_rays, int n_samples, float near_plane,
                                         float far_plane, const float* bg, int64_t bg_rows, int64_t chunk_rays, void* workspace,
                                         float* out_rgb, float* out_depth, float* out_acc, nerf_stream_t stream) {
  NERF_REQUIRE(n_rays >= 0, "nerf_render_rays_grid_fwd: n_rays=%lld", (long long)n_rays);
  if (n_rays == 0) return NERF_OK;
  NERF_REQUIRE(n_samples >= 2 && n_samples <= 1024 && chunk_rays > 0, "nerf_render_rays_grid_fwd: n_samples=%d (2..1024) chunk=%lld",
               n_samples, (long long)chunk_rays);
  NERF_REQUIRE(chunk_rays < ((int64_t)1 << 31) && chunk_rays * (int64_t)n_samples < ((int64_t)1 << 31),
               "nerf_render_rays_grid_fwd: chunk too large (chunk_rays * n_samples must stay below 2^31)");
  NERF_REQUIRE(grid_resolution > 0 && grid_resolution <= 32768 && grid_bound > 0.0f,
               "nerf_render_rays_grid_fwd: grid_resolution=%d (1..32768), grid_bound must be positive", grid_resolution);
  NERF_REQUIRE(bg == nullptr || bg_rows == 1 || bg_rows == n_rays, "nerf_render_rays_grid_fwd: bg_rows=%lld", (long long)bg_rows);
  NERF_REQUIRE(packed && binary_grid && rays_o && rays_d && workspace && out_rgb && out_depth && out_acc,
               "nerf_render_rays_grid_fwd: NULL pointer");
  NERF_REQUIRE(((uintptr_t)workspace & 255) == 0 && ((uintptr_t)packed & 255) == 0,
               "nerf_render_rays_grid_fwd: workspace and packed must be 256-byte aligned");
  // only the default inference kernel has a counted form: another family would not give nerf_mlp_fwd's bits under the same options
  NERF_REQUIRE(nerf::options().chain_legacy == 0, "nerf_render_rays_grid_fwd: option chain_legacy is set (the counted chain is the default kernel only)");
  NERF_REQUIRE(nerf::options().infer_shape32 == 0, "nerf_render_rays_grid_fwd: option infer_shape32 is set (the counted chain is the default kernel only)");
  NERF_REQUIRE(nerf::options().infer64 != 0, "nerf_render_rays_grid_fwd: option infer64 is 0 (the counted chain is the 64-samples-per-wave kernel only)");
  const GridRenderLayout l = grid_render_layout(chunk_rays, n_samples);
  char* w = static_cast<char*>(workspace);
  unsigned* count = reinterpret_cast<unsigned*>(w);
  float* z = reinterpret_cast<float*>(w + l.z);
  int* slots = reinterpret_cast<int*>(w + l.slots);
  float* pts = reinterpret_cast<float*>(w + l.pts);
  float* dirs = reinterpret_cast<float*>(w + l.dirs);
  float* rgb = reinterpret_cast<float*>(w + l.rgb);
  float* sigma = reinterpret_cast<float*>(w + l.sigma);
  const int64_t capacity = chunk_rays * (int64_t)n_samples;       // sizes the counted launch of EVERY chunk (the last may hold fewer rays)
  for (int64_t r0 = 0; r0 < n_rays; r0 += chunk_rays) {
    const int64_t r = n_rays - r0 < chunk_rays ? n_rays - r0 : chunk_rays;
    // (nerf_sample_compact clears the count word on the stream before its kernel adds to it)
    int rc = nerf_sample_compact(rays_o + r0 * 3, rays_d + r0 * 3, nullptr, r, n_samples, near_plane, far_plane, binary_grid, grid_resolution,
                                 grid_bound, z, slots, pts, dirs, count, stream);
    if (rc != NERF_OK) return rc;
    rc = nerf::mlp_fwd_counted(packed, pts, dirs, count, capacity, rgb, sigma, stream);
    if (rc != NERF_OK) return rc;
    rc = nerf_composite_fwd_indexed(rgb, sigma, slots, z, rays_d + r0 * 3, bg == nullptr ? nullptr : (bg_rows > 1 ? bg + r0 * 3 : bg),
                                    bg_rows > 1 ? r : bg_rows, r, n_samples, out_rgb + r0 * 3, out_depth + r0, out_acc + r0, stream);
    if (rc != NERF_OK) return rc;
  }
  return NERF_OK;
}
