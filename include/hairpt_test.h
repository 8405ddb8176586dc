/*
 * hairpt_test.h -- test hooks of libhairpt.so that are no part of the drop-in boundary
 * (hairpt.h): entry points that exist so a test can drive one production kernel with inputs
 * of its own, or read an intermediate result back.  Same conventions as hairpt.h (0 or a
 * negative HPT_E* code, hpt_last_error, caller-owned host buffers).
 */
#ifndef HAIRPT_TEST_H
#define HAIRPT_TEST_H
#include "hairpt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ImageBlock::put (include/mitsuba/render/imageblock.h:144-189) of caller-given samples through
   the production k_splat + k_gather of the context's filter (hpt_set_rfilter), on a prepared
   device context: pos is W*H*n_spp x 2 film positions (pixels), rgb W*H*n_spp x 3 radiance
   values, both pixel-major in image order -- sample j of pixel (x, y) at (y * W + x) * n_spp + j,
   and it must lie in that pixel, [x, x+1) x [y, y+1), as a camera sample does.  The samples of
   shard `shard` of `n_shards` are splatted in the waves an hpt_render of n_spp samples per pixel
   with this max_wave_paths would use, and ACCUMULATED into film_rgbw (W*H*4). */
int hpt_film_splat_batch(hpt_context *ctx, int n_spp, const float *pos, const float *rgb, int shard, int n_shards,
                         uint64_t max_wave_paths, float *film_rgbw);
/* The film position and radiance (the arguments of ImageBlock::put, src/librender/integrator.cpp:
   171-184) of every sample of the last hpt_render / hpt_render_device on this context, in the
   layout above; *n receives their number, W*H*(spp_end - spp_begin).  Pixels of blocks another
   shard owns are left untouched.  NULL pos and rgb only query n.  Valid when that render was one
   wave of paths (hpt_stats.waves == 1) and nothing has used the wave buffers since; otherwise
   HPT_ESTATE. */
int hpt_get_render_samples(hpt_context *ctx, float *pos, float *rgb, uint64_t *n);

#ifdef __cplusplus
}
#endif
#endif
