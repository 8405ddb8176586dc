/*
 * hpt_capi_batch.cpp -- the batch entry points of the C ABI (include/hairpt.h): single kernels
 * of the renderer run over arrays of the caller's inputs, for the tests that compare them with
 * the oracle one stage at a time.
 */
#include <algorithm>
#include <vector>

#include "hpt_context.h"

namespace {
struct Scratch {
    std::vector<void *> ptrs;
    ~Scratch() {
        for (void *p : ptrs) (void) hipFree(p);
    }
    template <typename T> T *in(const T *src, size_t n) {
        void *p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(n * sizeof(T), 16)) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        if (src && n) (void) hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
        return (T *) p;
    }
};
template <typename T> void fetch(T *dst, const T *src, size_t n) {
    if (dst) (void) hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost);
}
} // namespace
extern "C" {

int hpt_sobol_batch(hpt_context *c, int m, int n, const uint32_t *frame, const uint32_t *px, const uint32_t *py,
                    const uint32_t *dim, uint64_t *oi, float *ov) {
    if (!c || !c->prepared) return setErr(c, HPT_ESTATE, "prepare first");
    if (c->device == HPT_HOST_ONLY) return setErr(c, HPT_EDEVICE, "host-only context has no device");
    /* the kernel indexes the tables by m and dim: reject what they do not hold */
    const int rows = (int) std::min(c->vdc.size(), c->vdcInv.size()) / HPT_SOBOL_BITS;
    if (n < 0 || m < 0 || m > rows) return setErr(c, HPT_EINVAL, "Sobol look-up resolution out of range");
    for (int i = 0; i < n; ++i)
        if (dim[i] >= HPT_SOBOL_DIMS)
            return setErr(c, HPT_EINVAL, "Lookup dimension exceeds the direction number table size!");
    HIPCHK(c, hipSetDevice(c->device));
    Scratch S;
    const uint32_t *df = S.in(frame, n), *dx = S.in(px, n), *dy = S.in(py, n), *dd = S.in(dim, n);
    uint64_t *di = S.in<uint64_t>(nullptr, n);
    float *dv = S.in<float>(nullptr, n);
    HIPCHK(c, hpt_launch_sobol_batch(c->sc, m, n, df, dx, dy, dd, di, dv, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    fetch(oi, di, n);
    fetch(ov, dv, n);
    return HPT_OK;
}

int hpt_camera_batch(hpt_context *c, int n, const float *pos, float *oo, float *od, float *omint, float *omaxt) {
    if (!c || !c->prepared) return setErr(c, HPT_ESTATE, "prepare first");
    if (c->device == HPT_HOST_ONLY) return setErr(c, HPT_EDEVICE, "host-only context has no device");
    HIPCHK(c, hipSetDevice(c->device));
    Scratch S;
    const float *dp = S.in(pos, 2 * (size_t) n);
    float *o = S.in<float>(nullptr, 3 * (size_t) n), *d = S.in<float>(nullptr, 3 * (size_t) n);
    float *a = S.in<float>(nullptr, n), *b = S.in<float>(nullptr, n);
    HIPCHK(c, hpt_launch_camera_batch(c->sc, n, dp, o, d, a, b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    fetch(oo, o, 3 * (size_t) n);
    fetch(od, d, 3 * (size_t) n);
    fetch(omint, a, n);
    fetch(omaxt, b, n);
    return HPT_OK;
}

int hpt_trace_batch(hpt_context *c, int n, const float *o, const float *d, const float *mint, const float *maxt,
                    int flags, float *ot, int32_t *oiv, float *op, uint8_t *oh) {
    const int shadow = flags & HPT_TRACE_SHADOW;
    if (!c || !c->prepared) return setErr(c, HPT_ESTATE, "prepare first");
    if (c->device == HPT_HOST_ONLY) return setErr(c, HPT_EDEVICE, "host-only context has no device");
    HIPCHK(c, hipSetDevice(c->device));
    Scratch S;
    const float *a = S.in(o, 3 * (size_t) n), *b = S.in(d, 3 * (size_t) n), *mi = S.in(mint, n), *ma = S.in(maxt, n);
    float *dt = S.in<float>(nullptr, n), *dp = S.in<float>(nullptr, 3 * (size_t) n);
    int32_t *ds = S.in<int32_t>(nullptr, n);
    uint8_t *dh = S.in<uint8_t>(nullptr, n);
    uint32_t *cur = S.in<uint32_t>(nullptr, HPT_CURSORS * HPT_CURSOR_STRIDE);
    if (int rf = clearFault(c)) return rf;
    HIPCHK(c, hpt_launch_trace_batch(c->sc, n, a, b, mi, ma, flags, dt, ds, dp, dh, cur, c->stream));
    if (int rf = checkFault(c)) return rf;
    if (shadow) {
        fetch(oh, dh, n);
    } else {
        fetch(ot, dt, n);
        fetch(op, dp, 3 * (size_t) n);
        std::vector<int32_t> seg(n);
        fetch(seg.data(), ds, n);
        if (oiv)
            for (int i = 0; i < n; ++i) oiv[i] = seg[i] < 0 ? -1 : (int32_t) c->tree.segFirstVertex[seg[i]];
    }
    return HPT_OK;
}

int hpt_bsdf_batch(hpt_context *c, int n, const float *wi, const float *wo, const float *u, float *oe, float *op,
                   float *owo, float *ow, float *osp, uint32_t *ot) {
    if (!c || !c->prepared) return setErr(c, HPT_ESTATE, "prepare first");
    if (c->device == HPT_HOST_ONLY) return setErr(c, HPT_EDEVICE, "host-only context has no device");
    HIPCHK(c, hipSetDevice(c->device));
    Scratch S;
    const float *a = S.in(wi, 3 * (size_t) n), *b = S.in(wo, 3 * (size_t) n), *uu = S.in(u, 2 * (size_t) n);
    float *de = S.in<float>(nullptr, 3 * (size_t) n), *dp = S.in<float>(nullptr, n);
    float *dwo = S.in<float>(nullptr, 3 * (size_t) n), *dw = S.in<float>(nullptr, 3 * (size_t) n);
    float *dsp = S.in<float>(nullptr, n);
    uint32_t *dt = S.in<uint32_t>(nullptr, n);
    HIPCHK(c, hpt_launch_bsdf_batch(c->sc, n, a, b, uu, de, dp, dwo, dw, dsp, dt, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    fetch(oe, de, 3 * (size_t) n);
    fetch(op, dp, n);
    fetch(owo, dwo, 3 * (size_t) n);
    fetch(ow, dw, 3 * (size_t) n);
    fetch(osp, dsp, n);
    fetch(ot, dt, n);
    return HPT_OK;
}

int hpt_env_batch(hpt_context *c, int n, const float *refp, const float *u, const float *dq, float *od, float *ov,
                  float *op, float *odist, float *oe, float *oep) {
    if (!c || !c->prepared) return setErr(c, HPT_ESTATE, "prepare first");
    if (c->device == HPT_HOST_ONLY) return setErr(c, HPT_EDEVICE, "host-only context has no device");
    HIPCHK(c, hipSetDevice(c->device));
    Scratch S;
    const float *a = S.in(refp, 3 * (size_t) n), *uu = S.in(u, 2 * (size_t) n), *q = S.in(dq, 3 * (size_t) n);
    float *dd = S.in<float>(nullptr, 3 * (size_t) n), *dv = S.in<float>(nullptr, 3 * (size_t) n);
    float *dp = S.in<float>(nullptr, n), *ddist = S.in<float>(nullptr, n), *de = S.in<float>(nullptr, 3 * (size_t) n);
    float *dep = S.in<float>(nullptr, n);
    HIPCHK(c, hpt_launch_env_batch(c->sc, n, a, uu, q, dd, dv, dp, ddist, de, dep, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    fetch(od, dd, 3 * (size_t) n);
    fetch(ov, dv, 3 * (size_t) n);
    fetch(op, dp, n);
    fetch(odist, ddist, n);
    fetch(oe, de, 3 * (size_t) n);
    fetch(oep, dep, n);
    return HPT_OK;
}

int hpt_env_eval_filtered(hpt_context *c, int n, const float *d, const float *rx, const float *ry, float *out_rgb) {
    if (!c || !c->prepared) return setErr(c, HPT_ESTATE, "prepare first");
    if (c->device == HPT_HOST_ONLY) return setErr(c, HPT_EDEVICE, "host-only context has no device");
    HIPCHK(c, hipSetDevice(c->device));
    Scratch S;
    const float *a = S.in(d, 3 * (size_t) n), *b = S.in(rx, 3 * (size_t) n), *q = S.in(ry, 3 * (size_t) n);
    float *dout = S.in<float>(nullptr, 3 * (size_t) n);
    HIPCHK(c, hpt_launch_env_filtered_batch(c->sc, n, a, b, q, dout, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    fetch(out_rgb, dout, 3 * (size_t) n);
    return HPT_OK;
}

int hpt_get_env_level(hpt_context *c, int level, float *rgb, int *w, int *h) {
    if (!c || !c->prepared) return setErr(c, HPT_ESTATE, "prepare first");
    const int n = (int) c->env.levelW.size();
    if (level < 0 || level >= n) return n;
    if (w) *w = c->env.levelW[level];
    if (h) *h = c->env.levelH[level];
    if (rgb) {
        const HptF4 *t = &c->env.mip[c->env.levelOff[level]];
        for (size_t i = 0; i < (size_t) c->env.levelW[level] * c->env.levelH[level]; ++i) {
            rgb[3 * i] = t[i].x;
            rgb[3 * i + 1] = t[i].y;
            rgb[3 * i + 2] = t[i].z;
        }
    }
    return n;
}

} /* extern "C" */
