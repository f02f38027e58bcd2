// Evaluation entry of Part 3 with a hash-grid canonical field (canonical_type: instant): the counted render chain of render_counted.h
// with three field launches at ONE time stamp -- the deformation MLP on the compact points, the fp16 gather of the canonical table at
// x_c, the canonical chain (p3_deform_counted, hash_fwd_counted_f16, p4_canon_fwd_counted: common.h).  The operand piece of the
// workspace holds x_c [roundup(n, 128), 3] fp32, then the fp16 canonical image [roundup(n, 128), 32]: 76 bytes per row, the only pieces
// of the two training workspaces inference needs.  Host code only.
#include "render_counted.h"

static const char* const kWhat = "nerf_p3_render_rays_fwd";
static const size_t kXcRowBytes = 3 * 4, kImageRowBytes = 32 * 2;            // x_c fp32; 16 levels x 2 features, fp16
static const size_t kOperandRowBytes = kXcRowBytes + kImageRowBytes;

extern "C" size_t nerf_p3_render_workspace_bytes(int64_t chunk_rays, int n_samples) {
  return nerf::counted_render_workspace_bytes(chunk_rays, n_samples, kOperandRowBytes);
}

extern "C" int nerf_p3_render_rays_fwd(const void* packed_deform, const void* packed_canon, const float* table_f32, const void* table_f16,
                                       int canon_levels, const float* scale_host, const unsigned* res_host, const unsigned* size_host,
                                       const unsigned* offset_host, const unsigned* dense_host, float hash_bound,
                                       const uint8_t* binary_grid, int grid_resolution, float grid_bound, const float* rays_o,
                                       const float* rays_d, int64_t n_rays, int n_samples, float near_plane, float far_plane,
                                       const float* time_dev, const float* bg, int64_t bg_rows, int64_t chunk_rays, void* workspace,
                                       float* out_rgb, float* out_depth, float* out_acc, nerf_stream_t stream) {
  NERF_REQUIRE(n_rays >= 0, "%s: n_rays=%lld", kWhat, (long long)n_rays);
  if (n_rays == 0) return NERF_OK;
  NERF_REQUIRE(canon_levels == 16, "%s: canon_levels=%d (the canonical chain reads 16 levels x 2 features)", kWhat, canon_levels);
  NERF_REQUIRE((table_f32 == nullptr) != (table_f16 == nullptr), "%s: exactly one of table_f32 / table_f16", kWhat);
  NERF_REQUIRE(hash_bound > 0.0f && grid_bound > 0.0f, "%s: hash_bound and grid_bound must be positive", kWhat);
  NERF_REQUIRE(packed_deform && packed_canon && scale_host && res_host && size_host && offset_host && dense_host && time_dev,
               "%s: NULL pointer", kWhat);
  const nerf::LevelArgs levels{canon_levels, scale_host, res_host, size_host, offset_host, dense_host, hash_bound};
  return nerf::counted_render(
      kWhat, kOperandRowBytes, binary_grid, grid_resolution, grid_bound, rays_o, rays_d, n_rays, n_samples, near_plane, far_plane, bg, bg_rows,
      chunk_rays, workspace, out_rgb, out_depth, out_acc, stream,
      [=](const float* pts, const float* dirs, const unsigned* count, int64_t capacity, void* operands, float* rgb, float* sigma) {
        float* xc = static_cast<float*>(operands);
        void* image = static_cast<char*>(operands) + (size_t)((capacity + 127) / 128 * 128) * kXcRowBytes;
        int rc = nerf::p3_deform_counted(packed_deform, pts, count, capacity, time_dev, xc, stream);
        if (rc != NERF_OK) return rc;
        rc = nerf::hash_fwd_counted_f16(xc, count, capacity, table_f32, table_f16, levels, image, stream);
        if (rc != NERF_OK) return rc;
        return nerf::p4_canon_fwd_counted(packed_canon, image, dirs, count, capacity, time_dev, rgb, sigma, stream);
      });
}
