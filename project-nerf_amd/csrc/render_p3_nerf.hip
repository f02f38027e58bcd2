// Evaluation entry of Part 3 with the 8x256 canonical field (canonical_type: nerf, standard and direct time conditioning): a frame at
// ONE time as one launch chain (reference render_image, src/renderer.py:387-418, on the Part 3 forward of NeuralField,
// src/core.py:108-146).  This field has no occupancy grid, so a frame is dense and every row count is known on the host; per chunk
// nerf_sample_rays (plain depths, pts and dirs) -> the deformation chain at the scalar time on every row (p3_deform_rows; skipped
// under direct time conditioning) -> the canonical chain at x_c (at pts under direct time conditioning) and the scalar time
// (p3_canon_fwd_scalar_time) -> nerf_composite_fwd, on the caller's stream in ONE caller-provided workspace: no allocation, no host
// read, no synchronisation, graph-capturable.  Host code only.
#include "common.h"

static const char* const kWhat = "nerf_p3_nerf_render_rays_fwd";

namespace {
struct Layout {
  size_t z, pts, dirs, xc, sigma, rgb, total;
};
// one formula, one layout: x_c is laid out under direct time conditioning too
Layout layout(int64_t chunk_rays, int n_samples) {
  const size_t n = (size_t)chunk_rays * (size_t)n_samples;
  Layout l{};
  size_t o = 0;
  l.z = nerf::piece(&o, n * 4);
  l.pts = nerf::piece(&o, n * 12);
  l.dirs = nerf::piece(&o, n * 12);
  l.xc = nerf::piece(&o, n * 12);
  l.sigma = nerf::piece(&o, n * 4);
  l.rgb = nerf::piece(&o, n * 12);
  l.total = o;
  return l;
}
}  // namespace

extern "C" size_t nerf_p3_nerf_render_workspace_bytes(int64_t chunk_rays, int n_samples) {
  if (chunk_rays <= 0 || n_samples <= 0) return 0;
  return layout(chunk_rays, n_samples).total;
}

extern "C" int nerf_p3_nerf_render_rays_fwd(const void* packed_deform, const void* packed_canon, const float* rays_o, const float* rays_d,
                                            int64_t n_rays, int n_samples, float near_plane, float far_plane, const float* time_dev,
                                            const float* bg, int64_t bg_rows, int64_t chunk_rays, void* workspace, float* out_rgb,
                                            float* out_depth, float* out_acc, nerf_stream_t stream) {
  NERF_REQUIRE(n_rays >= 0, "%s: n_rays=%lld", kWhat, (long long)n_rays);
  if (n_rays == 0) return NERF_OK;
  NERF_REQUIRE(n_samples >= 2 && n_samples <= 1024, "%s: n_samples=%d (2..1024)", kWhat, n_samples);
  NERF_REQUIRE(chunk_rays > 0, "%s: chunk_rays=%lld", kWhat, (long long)chunk_rays);
  NERF_REQUIRE(chunk_rays < ((int64_t)1 << 31) && chunk_rays * (int64_t)n_samples < ((int64_t)1 << 31), "%s: chunk too large", kWhat);
  NERF_REQUIRE(packed_canon && rays_o && rays_d && time_dev && workspace && out_rgb && out_depth && out_acc, "%s: NULL pointer", kWhat);
  NERF_REQUIRE(((uintptr_t)workspace & 255) == 0, "%s: workspace must be 256-byte aligned", kWhat);
  NERF_REQUIRE(((uintptr_t)packed_canon & 255) == 0, "%s: packed_canon must be 256-byte aligned", kWhat);
  NERF_REQUIRE(bg == nullptr || bg_rows == 1 || bg_rows == n_rays, "%s: bg_rows=%lld", kWhat, (long long)bg_rows);
  const Layout l = layout(chunk_rays, n_samples);
  char* w = static_cast<char*>(workspace);
  float* z = reinterpret_cast<float*>(w + l.z);
  float* pts = reinterpret_cast<float*>(w + l.pts);
  float* dirs = reinterpret_cast<float*>(w + l.dirs);
  float* xc = reinterpret_cast<float*>(w + l.xc);
  float* sigma = reinterpret_cast<float*>(w + l.sigma);
  float* rgb = reinterpret_cast<float*>(w + l.rgb);
  for (int64_t r0 = 0; r0 < n_rays; r0 += chunk_rays) {
    const int64_t r = n_rays - r0 < chunk_rays ? n_rays - r0 : chunk_rays;
    const int64_t n = r * n_samples;
    int rc = nerf_sample_rays(rays_o + r0 * 3, rays_d + r0 * 3, nullptr, r, n_samples, near_plane, far_plane, z, pts, dirs, stream);
    if (rc != NERF_OK) return rc;
    if (packed_deform != nullptr) {
      rc = nerf::p3_deform_rows(packed_deform, pts, n, time_dev, xc, stream);
      if (rc != NERF_OK) return rc;
    }
    rc = nerf::p3_canon_fwd_scalar_time(packed_canon, packed_deform != nullptr ? xc : pts, dirs, n, time_dev, rgb, sigma, stream);
    if (rc != NERF_OK) return rc;
    rc = nerf_composite_fwd(rgb, sigma, z, rays_d + r0 * 3, bg == nullptr ? nullptr : (bg_rows > 1 ? bg + r0 * 3 : bg), bg_rows > 1 ? r : bg_rows,
                            nullptr, r, n_samples, out_rgb + r0 * 3, out_depth + r0, out_acc + r0, nullptr, nullptr, stream);
    if (rc != NERF_OK) return rc;
  }
  return NERF_OK;
}
