/*
 * hpt_render_multi.cpp -- one frame over several devices of one process: every context renders
 * its shard (renderImpl, one host thread per context) and the films are combined on the first
 * context's device.
 */
#include <cstring>
#include <thread>

#include "hpt_context.h"

namespace {

/* one film from one scene: every context must be a share of the same prepared scene
   (re-preparing or re-configuring a context gives it a scene of its own), with the same
   camera and integrator settings and the same shard deal */
int checkSameScene(hpt_context *const *ctxs, int n) {
    hpt_context *c0 = ctxs[0];
    for (int g = 0; g < n; ++g) {
        const hpt_context *c = ctxs[g];
        if (!c) return HPT_EINVAL;
        if (c->device == HPT_HOST_ONLY) return setErr(c0, HPT_EDEVICE, "host-only context cannot render");
        if (!c->prepared) return setErr(c0, HPT_ESTATE, "hpt_render_multi: a context is not prepared");
        if (c->sceneId != c0->sceneId)
            return setErr(c0, HPT_EINVAL, "hpt_render_multi: context " + std::to_string(g) +
                                              " renders a different prepared scene (share one with hpt_context_share_scene)");
        if (std::memcmp(&c->sc.cam, &c0->sc.cam, sizeof(HptCamera)) != 0 || c->sc.maxDepth != c0->sc.maxDepth ||
            c->sc.rrDepth != c0->sc.rrDepth || c->sc.strictNormals != c0->sc.strictNormals ||
            c->sc.hideEmitters != c0->sc.hideEmitters || c->sc.scramble != c0->sc.scramble || c->desc.spp != c0->desc.spp)
            return setErr(c0, HPT_EINVAL, "hpt_render_multi: context " + std::to_string(g) +
                                              " has a different camera, sampler or integrator setting");
        if (std::memcmp(c->sc.filter, c0->sc.filter, sizeof(c->sc.filter)) != 0 || c->sc.filterScale != c0->sc.filterScale ||
            c->sc.filterRadius != c0->sc.filterRadius || c->sc.filterBorder != c0->sc.filterBorder)
            return setErr(c0, HPT_EINVAL, "hpt_render_multi: context " + std::to_string(g) +
                                              " has a different reconstruction filter (hpt_set_rfilter on every context)");
        if (c->blockWeights != c0->blockWeights)
            return setErr(c0, HPT_EINVAL, "hpt_render_multi: context " + std::to_string(g) +
                                              " deals the blocks with different weights (hpt_set_block_weights on every context)");
    }
    return HPT_OK;
}

/* the receiving context's copy streams: one (and its done event) per peer film */
int ensurePeerStreams(hpt_context *c0, int peers) {
    while ((int) c0->peerStreams.size() < peers) {
        hipStream_t ps;
        hipEvent_t pe;
        HIPCHK(c0, hipStreamCreateWithFlags(&ps, hipStreamNonBlocking));
        if (hipEventCreateWithFlags(&pe, hipEventDisableTiming) != hipSuccess) {
            (void) hipStreamDestroy(ps);
            return setErr(c0, HPT_EDEVICE, "hpt_render_multi: cannot create a copy event");
        }
        c0->peerStreams.push_back(ps);
        c0->peerEvents.push_back(pe);
    }
    return HPT_OK;
}

} // namespace

extern "C" {

int hpt_render_multi(hpt_context *const *ctxs, int n, const hpt_render_params *prm, float *film) {
    if (!ctxs || n <= 0 || !prm || !film) return HPT_EINVAL;
    hpt_context *c0 = ctxs[0];
    if (!c0) return HPT_EINVAL;
    if (int rc = checkSameScene(ctxs, n)) return rc;
    const size_t pixels = (size_t) c0->sc.cam.width * c0->sc.cam.height;
    /* every context renders its shard into its own device film; the receiving context's film
       starts as the caller's (hpt_render accumulates), the others at zero */
    std::vector<int> rcs(n, HPT_OK);
    auto shard = [&](int g) {
        hpt_context *c = ctxs[g];
        auto fail = [&](hipError_t e) { rcs[g] = setErr(c, HPT_EDEVICE, hipGetErrorString(e)); };
        hipError_t e = hipSetDevice(c->device);
        if (e == hipSuccess && c->mfilmPixels < pixels) {
            if (c->mfilm) (void) hipFree(c->mfilm);
            c->mfilm = nullptr;
            c->mfilmPixels = 0;
            e = hipMalloc((void **) &c->mfilm, pixels * 16);
            if (e == hipSuccess) c->mfilmPixels = pixels;
        }
        if (e == hipSuccess)
            e = g == 0 ? hipMemcpyAsync(c->mfilm, film, pixels * 16, hipMemcpyHostToDevice, c->stream)
                       : hipMemsetAsync(c->mfilm, 0, pixels * 16, c->stream);
        if (e != hipSuccess) return fail(e);
        hpt_render_params p = *prm;
        p.shard = g;
        p.n_shards = n;
        rcs[g] = renderImpl(c, &p, c->mfilm);
        /* the film is complete on this context's stream before the receiving device reads it */
        if (rcs[g] == HPT_OK && g > 0 && (e = hipStreamSynchronize(c->stream)) != hipSuccess) fail(e);
    };
    {
        std::vector<std::thread> th;
        for (int g = 1; g < n; ++g) th.emplace_back(shard, g);
        shard(0);
        for (auto &t : th) t.join();
    }
    for (int g = 0; g < n; ++g)
        if (rcs[g]) {
            if (g) setErr(c0, rcs[g], "device " + std::to_string(ctxs[g]->device) + ": " + ctxs[g]->err);
            return rcs[g];
        }
    /* the film combine (renderproc.cpp:142-145) on the receiving device: every other film is
       pulled at once over xGMI (peer copies, one stream and staging buffer per peer), then
       added in shard order, so the sum is the host sum f0 + f1 + ... of the same films */
    HIPCHK(c0, hipSetDevice(c0->device));
    if (n > 1) {
        const size_t need = (size_t) (n - 1) * pixels;
        if (c0->mstagePixels < need) {
            if (c0->mstage) (void) hipFree(c0->mstage);
            c0->mstage = nullptr;
            c0->mstagePixels = 0;
            HIPCHK(c0, hipMalloc((void **) &c0->mstage, need * 16));
            c0->mstagePixels = need;
        }
        if (int rc = ensurePeerStreams(c0, n - 1)) return rc;
        for (int g = 1; g < n; ++g) {
            const int dg = ctxs[g]->device;
            if (dg != c0->device) {
                int can = 0;
                HIPCHK(c0, hipDeviceCanAccessPeer(&can, c0->device, dg));
                if (!can)
                    return setErr(c0, HPT_EDEVICE, "hpt_render_multi: device " + std::to_string(c0->device) +
                                                       " cannot access device " + std::to_string(dg) + " (no peer path)");
                const hipError_t pe = hipDeviceEnablePeerAccess(dg, 0);
                if (pe == hipErrorPeerAccessAlreadyEnabled) (void) hipGetLastError(); /* enabled by an earlier call */
                else if (pe != hipSuccess)
                    return setErr(c0, HPT_EDEVICE, "hipDeviceEnablePeerAccess(" + std::to_string(dg) +
                                                       "): " + hipGetErrorString(pe));
            }
            float4 *stage = c0->mstage + (size_t) (g - 1) * pixels;
            HIPCHK(c0, hipMemcpyPeerAsync(stage, c0->device, ctxs[g]->mfilm, dg, pixels * 16, c0->peerStreams[g - 1]));
            HIPCHK(c0, hipEventRecord(c0->peerEvents[g - 1], c0->peerStreams[g - 1]));
        }
        for (int g = 1; g < n; ++g) {
            HIPCHK(c0, hipStreamWaitEvent(c0->stream, c0->peerEvents[g - 1], 0));
            HIPCHK(c0, hpt_launch_film_add(c0->mfilm, c0->mstage + (size_t) (g - 1) * pixels, pixels, c0->stream));
        }
    }
    HIPCHK(c0, hipMemcpyAsync(film, c0->mfilm, pixels * 16, hipMemcpyDeviceToHost, c0->stream));
    HIPCHK(c0, hipStreamSynchronize(c0->stream));
    return HPT_OK;
}

} /* extern "C" */
