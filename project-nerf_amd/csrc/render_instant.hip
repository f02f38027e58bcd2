// Evaluation entry of the Instant-NGP field: the counted render chain of render_counted.h with the hash gather and the tiny-MLP
// chain (hash_fwd_counted, imlp_fwd_counted: common.h) as its two field launches, the bf16 hash operand image between them -- the
// only piece of the training workspace inference needs.  Host code only.
#include "render_counted.h"

static const char* const kWhat = "nerf_instant_render_rays_fwd";
static const size_t kImageRowBytes = 32 * 2;            // 16 levels x 2 features, bf16

extern "C" size_t nerf_instant_render_workspace_bytes(int64_t chunk_rays, int n_samples) {
  return nerf::counted_render_workspace_bytes(chunk_rays, n_samples, kImageRowBytes);
}

extern "C" int nerf_instant_render_rays_fwd(const void* imlp_packed, const float* table_f32, const void* table_f16, int n_levels,
                                            const float* scale_host, const unsigned* res_host, const unsigned* size_host,
                                            const unsigned* offset_host, const unsigned* dense_host, float hash_bound,
                                            const uint8_t* binary_grid, int grid_resolution, float grid_bound, const float* rays_o,
                                            const float* rays_d, int64_t n_rays, int n_samples, float near_plane, float far_plane,
                                            const float* bg, int64_t bg_rows, int64_t chunk_rays, void* workspace, float* out_rgb,
                                            float* out_depth, float* out_acc, nerf_stream_t stream) {
  NERF_REQUIRE(n_rays >= 0, "%s: n_rays=%lld", kWhat, (long long)n_rays);
  if (n_rays == 0) return NERF_OK;
  NERF_REQUIRE(n_levels == 16, "%s: n_levels=%d (the default-shape decoder chain reads 16 levels x 2 features)", kWhat, n_levels);
  NERF_REQUIRE((table_f32 == nullptr) != (table_f16 == nullptr), "%s: exactly one of table_f32 / table_f16", kWhat);
  NERF_REQUIRE(hash_bound > 0.0f, "%s: hash_bound must be positive", kWhat);
  NERF_REQUIRE(imlp_packed && scale_host && res_host && size_host && offset_host && dense_host, "%s: NULL pointer", kWhat);
  const nerf::LevelArgs levels{n_levels, scale_host, res_host, size_host, offset_host, dense_host, hash_bound};
  return nerf::counted_render(
      kWhat, kImageRowBytes, binary_grid, grid_resolution, grid_bound, rays_o, rays_d, n_rays, n_samples, near_plane, far_plane, bg, bg_rows,
      chunk_rays, workspace, out_rgb, out_depth, out_acc, stream,
      [=](const float* pts, const float* dirs, const unsigned* count, int64_t capacity, void* image, float* rgb, float* sigma) {
        const int rc = nerf::hash_fwd_counted(pts, count, capacity, table_f32, table_f16, levels, image, stream);
        if (rc != NERF_OK) return rc;
        return nerf::imlp_fwd_counted(imlp_packed, image, dirs, count, capacity, rgb, sigma, stream);
      });
}
