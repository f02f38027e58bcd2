// Evaluation entry of the vanilla (8x256) field through an occupancy grid: the counted render chain of render_counted.h with the
// inference chain in point mode (mlp_fwd_counted: common.h) as its one field launch and no operand image.  Host code only.
#include "render_counted.h"

static const char* const kWhat = "nerf_render_rays_grid_fwd";

extern "C" size_t nerf_render_rays_grid_workspace_bytes(int64_t chunk_rays, int n_samples) {
  return nerf::counted_render_workspace_bytes(chunk_rays, n_samples, 0);
}

extern "C" int nerf_render_rays_grid_fwd(const void* packed, const uint8_t* binary_grid, int grid_resolution, float grid_bound,
                                         const float* rays_o, const float* rays_d, int64_t n_rays, int n_samples, float near_plane,
                                         float far_plane, const float* bg, int64_t bg_rows, int64_t chunk_rays, void* workspace,
                                         float* out_rgb, float* out_depth, float* out_acc, nerf_stream_t stream) {
  NERF_REQUIRE(n_rays >= 0, "%s: n_rays=%lld", kWhat, (long long)n_rays);
  if (n_rays == 0) return NERF_OK;
  NERF_REQUIRE(packed != nullptr, "%s: NULL pointer", kWhat);
  NERF_REQUIRE(((uintptr_t)packed & 255) == 0, "%s: packed must be 256-byte aligned", kWhat);
  // only the default inference kernel has a counted form: another family would not give nerf_mlp_fwd's bits under the same options
  NERF_REQUIRE(nerf::options().chain_legacy == 0, "%s: option chain_legacy is set (the counted chain is the default kernel only)", kWhat);
  NERF_REQUIRE(nerf::options().infer_shape32 == 0, "%s: option infer_shape32 is set (the counted chain is the default kernel only)", kWhat);
  NERF_REQUIRE(nerf::options().infer64 != 0, "%s: option infer64 is 0 (the counted chain is the 64-samples-per-wave kernel only)", kWhat);
  return nerf::counted_render(kWhat, 0, binary_grid, grid_resolution, grid_bound, rays_o, rays_d, n_rays, n_samples, near_plane, far_plane,
                              bg, bg_rows, chunk_rays, workspace, out_rgb, out_depth, out_acc, stream,
                              [=](const float* pts, const float* dirs, const unsigned* count, int64_t capacity, void*, float* rgb,
                                  float* sigma) { return nerf::mlp_fwd_counted(packed, pts, dirs, count, capacity, rgb, sigma, stream); });
}
