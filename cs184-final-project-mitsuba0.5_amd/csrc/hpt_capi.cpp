/*
 * hpt_capi.cpp -- the C ABI (include/hairpt.h): the context's lifecycle, the scene setters and
 * getters, hpt_prepare and the upload of the prepared scene.  The wavefront driver behind
 * hpt_render is hpt_render_driver.cpp, hpt_render_multi hpt_render_multi.cpp, the batch entry
 * points of the tests hpt_capi_batch.cpp; hpt_context.h is what they share.
 */
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <stdexcept>

#include "hpt_context.h"

/* live paths below which a frame's remaining bounces run as one k_tail
   launch (HPT_TAIL_PATHS overrides; 0 keeps the per-bounce launches) */
uint32_t defaultTailPaths() {
    const char *v = std::getenv("HPT_TAIL_PATHS");
    return v ? (uint32_t) std::strtoul(v, nullptr, 10) : (1u << 17);
}

/* camera rays traced as 64-ray packets (k_trace_packet); HPT_PACKETS=0 traces them one per lane */
bool defaultPackets() {
    const char *v = std::getenv("HPT_PACKETS");
    return v ? std::atoi(v) != 0 : true;
}

/* device-side bounce control (launch a wave's bounces ahead without reading queue lengths
   back); HPT_BOUNCE_AHEAD=0 reads every bounce's queue length on the host */
bool defaultBounceAhead() {
    const char *v = std::getenv("HPT_BOUNCE_AHEAD");
    return v ? std::atoi(v) != 0 : true;
}

/* test hook: HPT_SCHEDULE_TEST=1 records schedules with half the queue lengths (the bounces
   launched ahead outgrow their grids: the wave is rendered again), =2 ends them one wavefront
   bounce early (the tail launched ahead finds too many live paths and leaves the bounce to
   k_shade: the host goes on bounce by bounce) */
int scheduleTestHook() {
    const char *v = std::getenv("HPT_SCHEDULE_TEST");
    return v ? std::atoi(v) : 0;
}

namespace {
/* HptBsdf::kind / hpt_scene_info::bsdf numbering */
int bsdfKindOf(const std::string &b) {
    if (b == "marschner") return HPT_BSDF_MARSCHNER;
    if (b == "kajiyakay") return HPT_BSDF_KAJIYAKAY;
    if (b == "roughplastic") return HPT_BSDF_ROUGHPLASTIC;
    if (b == "marschnerdielectric") return HPT_BSDF_MARSCHNERDIELECTRIC;
    if (b == "thindielectric") return HPT_BSDF_THINDIELECTRIC;
    if (b == "diffuse") return HPT_BSDF_DIFFUSE;
    return -1;
}
/* the low-level setters describe a single BSDF used by every shape */
BsdfDesc &singleBsdf(SceneDesc &d, const char *type) {
    d.bsdfs.assign(1, BsdfDesc());
    for (auto &h : d.shapes) h.bsdf = 0;
    d.bsdfs[0].type = type;
    return d.bsdfs[0];
}

/* errors of calls that have no context of their own to report on (hpt_context_create,
   hpt_context_share_scene): per calling thread, read with hpt_last_error(NULL) */
thread_local std::string tlsErr;

std::string defaultDataDir() {
    Dl_info info;
    if (dladdr((void *) &defaultDataDir, &info) && info.dli_fname) {
        std::string p = info.dli_fname;
        size_t s = p.find_last_of('/');
        std::string dir = s == std::string::npos ? "." : p.substr(0, s);
        return dir + "/../data";
    }
    return "data";
}

template <typename T> bool readFile(const std::string &path, std::vector<T> &out) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) return false;
    size_t n = (size_t) f.tellg();
    f.seekg(0);
    out.resize(n / sizeof(T));
    f.read((char *) out.data(), (std::streamsize) (out.size() * sizeof(T)));
    return (bool) f;
}

/* the film filter of c->desc into the kernels' scene record (setupFilter) */
int configureFilter(hpt_context *c) {
    std::string err;
    const SceneDesc &d = c->desc;
    if (!setupFilter(filterTypeOf(d.rfilter), d.rfilterP0, d.rfilterP1, c->sc.filter, c->sc.filterScale,
                     c->sc.filterRadius, c->sc.filterBorder, err))
        return setErr(c, HPT_EINVAL, err);
    return HPT_OK;
}

} // namespace

int setErr(hpt_context *c, int code, const std::string &m) {
    if (c) c->err = m;
    else tlsErr = m;
    return code;
}

int upload(hpt_context *c, const void *src, size_t bytes, const void **dst) {
    if (c->device == HPT_HOST_ONLY) { /* keep host pointers: nothing leaves the host */
        *dst = src;
        return HPT_OK;
    }
    DevBuf b;
    b.bytes = std::max<size_t>(bytes, 16);
    HIPCHK(c, hipMalloc(&b.p, b.bytes));
    if (bytes) HIPCHK(c, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    c->sceneBufs.push_back(b);
    *dst = b.p;
    return HPT_OK;
}

void freeBufs(std::vector<DevBuf> &v) {
    for (auto &b : v)
        if (b.p) (void) hipFree(b.p);
    v.clear();
}

/* the traversal-bound fault word (HptScene::fault): cleared before a call's
   launches, read after them; a set bit fails the call */
int clearFault(hpt_context *c) {
    HIPCHK(c, hipMemsetAsync(c->sc.fault, 0, 4, c->stream));
    return HPT_OK;
}
int checkFault(hpt_context *c) {
    uint32_t f = 0;
    HIPCHK(c, hipMemcpyAsync(&f, c->sc.fault, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (f & HPT_FAULT_LEAVES)
        return setErr(c, HPT_ETRAVERSAL, "kd-tree traversal exceeded 2^18 leaf rounds for a ray (malformed tree?)");
    if (f & HPT_FAULT_RESTARTS)
        return setErr(c, HPT_ETRAVERSAL, "kd-tree traversal exceeded its kd-restart bound for a ray");
    return HPT_OK;
}

hipEvent_t takeEvent(hpt_context *c, size_t &used) {
    if (used >= c->evPool.size()) {
        hipEvent_t e;
        (void) hipEventCreate(&e);
        c->evPool.push_back(e);
    }
    return c->evPool[used++];
}

extern "C" {

int hpt_context_create(int device, hpt_context **out) {
    tlsErr.clear(); /* hpt_last_error(NULL) describes this call only */
    if (!out) return HPT_EINVAL;
    *out = nullptr;
    if (device == HPT_HOST_ONLY) {
        /* host-only context: parses, loads, builds and exports the scene
           (kd-tree, tables) for inspection; every render / batch call fails */
        hpt_context *c = new hpt_context();
        c->device = HPT_HOST_ONLY;
        c->dataDir = defaultDataDir();
        std::memset(&c->sc, 0, sizeof(c->sc));
        std::memset(&c->stats, 0, sizeof(c->stats));
        *out = c;
        return HPT_OK;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return setErr(nullptr, HPT_EDEVICE, "no HIP device");
    if (device < 0 || device >= n)
        return setErr(nullptr, HPT_EINVAL, "device " + std::to_string(device) + " of " + std::to_string(n));
    if (hipSetDevice(device) != hipSuccess) return setErr(nullptr, HPT_EDEVICE, "hipSetDevice failed");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess)
        return setErr(nullptr, HPT_EDEVICE, "hipGetDeviceProperties failed");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return setErr(nullptr, HPT_EDEVICE, std::string("not a gfx950 device: ") + prop.gcnArchName);
    hpt_context *c = new hpt_context();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipHostMalloc((void **) &c->hostCnt, HPT_Q_COUNT * 4, hipHostMallocDefault) != hipSuccess) {
        delete c;
        return setErr(nullptr, HPT_EDEVICE, "stream / pinned counter allocation failed");
    }
    c->dataDir = defaultDataDir();
    std::memset(&c->sc, 0, sizeof(c->sc));
    std::memset(&c->stats, 0, sizeof(c->stats));
    *out = c;
    return HPT_OK;
}

void hpt_context_destroy(hpt_context *c) {
    if (!c) return;
    if (c->device == HPT_HOST_ONLY) {
        delete c;
        return;
    }
    (void) hipSetDevice(c->device);
    (void) hipStreamSynchronize(c->stream);
    freeBufs(c->sceneBufs);
    freeBufs(c->waveBufs);
    if (c->partial) (void) hipFree(c->partial);
    if (c->dBlockOf) (void) hipFree(c->dBlockOf);
    if (c->dLocalOf) (void) hipFree(c->dLocalOf);
    if (c->dBlockCost) (void) hipFree(c->dBlockCost);
    if (c->scDev) (void) hipFree(c->scDev);
    if (c->mfilm) (void) hipFree(c->mfilm);
    if (c->mstage) (void) hipFree(c->mstage);
    for (auto e : c->evPool) (void) hipEventDestroy(e);
    for (auto e : c->peerEvents) (void) hipEventDestroy(e);
    for (auto ps : c->peerStreams) (void) hipStreamDestroy(ps);
    (void) hipHostFree(c->hostCnt);
    (void) hipStreamDestroy(c->stream);
    delete c;
}

const char *hpt_last_error(const hpt_context *c) {
    if (c) return c->err.c_str();
    return tlsErr.empty() ? "null context" : tlsErr.c_str();
}

int hpt_set_data_dir(hpt_context *c, const char *dir) {
    if (!c || !dir) return HPT_EINVAL;
    c->dataDir = dir;
    return HPT_OK;
}

/* the process-wide -D table (hpt_set_default_defines) */
static std::mutex gDefinesMutex;
static std::map<std::string, std::string> gDefaultDefines;

int hpt_set_default_defines(int n_defines, const char *const *keys, const char *const *values) {
    if (n_defines < 0 || (n_defines > 0 && (!keys || !values))) return HPT_EINVAL;
    for (int i = 0; i < n_defines; ++i)
        if (!keys[i] || !values[i]) return HPT_EINVAL;
    std::lock_guard<std::mutex> lock(gDefinesMutex);
    gDefaultDefines.clear();
    for (int i = 0; i < n_defines; ++i) gDefaultDefines[keys[i]] = values[i];
    return HPT_OK;
}

int hpt_load_scene_xml(hpt_context *c, const char *path, int n_defines, const char *const *keys,
                       const char *const *values) {
    if (!c || !path) return HPT_EINVAL;
    /* the same argument checks as hpt_set_default_defines, before the context is touched */
    if (n_defines < 0 || (n_defines > 0 && (!keys || !values)))
        return setErr(c, HPT_EINVAL, "bad defines: n_defines < 0 or NULL key / value arrays");
    for (int i = 0; i < n_defines; ++i)
        if (!keys[i] || !values[i]) return setErr(c, HPT_EINVAL, "bad defines: NULL key or value");
    std::map<std::string, std::string> defs;
    {
        std::lock_guard<std::mutex> lock(gDefinesMutex);
        defs = gDefaultDefines;
    }
    for (int i = 0; i < n_defines; ++i) defs[keys[i]] = values[i]; /* explicit defines win */
    try {
        c->desc = parseSceneXML(path, defs);
    } catch (const std::exception &e) {
        return setErr(c, HPT_EIO, e.what());
    }
    const SceneDesc &d = c->desc;
    c->haveCamera = true;
    c->hairFromFile = true;
    c->haveHair = true;
    c->haveBSDF = true;
    c->haveEnv = true;
    c->envFromSunsky = d.emitter == "sunsky";
    if (d.emitter == "envmap") {
        std::string err;
        c->env = EnvHost();
        if (!loadEnvFile(d.envFile, c->env, err)) return setErr(c, HPT_EIO, err);
        c->env.scale = d.envScale;
        std::memcpy(c->env.toWorld, d.emitterToWorld, sizeof(c->env.toWorld));
    }
    c->prepared = false;
    return HPT_OK;
}

int hpt_export_scene_json(hpt_context *c, char *buf, size_t capacity, size_t *needed) {
    if (!c) return HPT_EINVAL;
    if (!c->hairFromFile) return setErr(c, HPT_ESTATE, "no scene loaded with hpt_load_scene_xml");
    const std::string js = sceneToJSON(c->desc);
    if (needed) *needed = js.size() + 1;
    if (!buf) return HPT_OK;
    if (capacity < js.size() + 1) return setErr(c, HPT_EINVAL, "buffer too small");
    std::memcpy(buf, js.c_str(), js.size() + 1);
    return HPT_OK;
}

int hpt_set_camera(hpt_context *c, const float to_world[16], float fov_x_deg, int width, int height,
                   float near_clip, float far_clip) {
    if (!c || !to_world || width <= 0 || height <= 0 || !(near_clip > 0) || !(near_clip < far_clip))
        return setErr(c, HPT_EINVAL, "invalid camera parameters");
    std::memcpy(c->desc.toWorld, to_world, sizeof(c->desc.toWorld));
    c->desc.fov = fov_x_deg;
    c->desc.fovAxis = "x";
    c->desc.width = width;
    c->desc.height = height;
    c->desc.nearClip = near_clip;
    c->desc.farClip = far_clip;
    c->haveCamera = true;
    c->prepared = false;
    return HPT_OK;
}

int hpt_set_sampler(hpt_context *c, int spp) {
    if (!c || spp <= 0) return setErr(c, HPT_EINVAL, "sampleCount must be positive");
    c->desc.spp = spp;
    return HPT_OK;
}

int hpt_set_sampler_scramble(hpt_context *c, uint64_t scramble) {
    if (!c) return HPT_EINVAL;
    c->desc.scramble = scramble;
    c->prepared = false;
    return HPT_OK;
}

int hpt_debug_sfmt(uint64_t seed, uint64_t n, uint64_t *out) {
    if (!out && n) return HPT_EINVAL;
    sfmtULongs(seed, (size_t) n, out);
    return HPT_OK;
}

int hpt_debug_fresnel_diffuse(int n, const float *eta, float *out) {
    if (n < 0 || (n > 0 && (!eta || !out))) return HPT_EINVAL;
    for (int i = 0; i < n; ++i) out[i] = fresnelDiffuseReflectance(eta[i]);
    return HPT_OK;
}

int hpt_set_traversal_bounds(hpt_context *c, uint32_t max_leaf_rounds, uint32_t max_restarts) {
    if (!c || max_leaf_rounds == 0) return HPT_EINVAL;
    c->maxLeafRounds = std::min<uint32_t>(max_leaf_rounds, HPT_MAX_LEAF_ROUNDS);
    c->maxRestarts = std::min<uint32_t>(max_restarts, HPT_MAX_RESTARTS);
    c->sc.maxLeafRounds = c->maxLeafRounds;
    c->sc.maxRestarts = c->maxRestarts;
    return HPT_OK;
}

int hpt_set_packet_stack(hpt_context *c, uint32_t entries) {
    if (!c) return HPT_EINVAL;
    c->packetStack = entries;
    c->sc.packetStack = entries;
    return HPT_OK;
}

int hpt_clear_schedules(hpt_context *c) {
    if (!c) return HPT_EINVAL;
    c->schedules.clear();
    return HPT_OK;
}

int hpt_set_integrator(hpt_context *c, int max_depth, int rr_depth, int strict_normals, int hide_emitters) {
    if (!c) return HPT_EINVAL;
    c->desc.maxDepth = max_depth;
    c->desc.rrDepth = rr_depth;
    c->desc.strictNormals = strict_normals != 0;
    c->desc.hideEmitters = hide_emitters != 0;
    c->prepared = false;
    return HPT_OK;
}

int hpt_set_hair_file(hpt_context *c, const char *path, float radius, float angle, const float *to_world) {
    if (!c || !path) return HPT_EINVAL;
    c->hairFromFile = true;
    HairShapeDesc h;
    h.file = path;
    h.radius = radius;
    h.angleThreshold = angle;
    h.hasToWorld = to_world != nullptr;
    if (to_world) std::memcpy(h.toWorld, to_world, sizeof(h.toWorld));
    c->desc.shapes.assign(1, h);
    c->haveHair = true;
    c->prepared = false;
    return HPT_OK;
}

int hpt_set_hair_reduction(hpt_context *c, float reduction) {
    if (!c) return HPT_EINVAL;
    if (!c->hairFromFile || c->desc.shapes.empty())
        return setErr(c, HPT_ESTATE, "hpt_set_hair_reduction: no hair file shape (hpt_set_hair_file first)");
    if (!(reduction >= 0 && reduction < 1))
        return setErr(c, HPT_EINVAL, "The 'reduction' parameter must have a value in [0, 1)!");
    c->desc.shapes.back().reduction = reduction;
    c->prepared = false;
    return HPT_OK;
}

int hpt_set_hair_vertices(hpt_context *c, const float *xyz, const uint8_t *starts, uint64_t n, float radius) {
    if (!c || (!xyz && n)) return HPT_EINVAL;
    c->hairFromFile = false;
    c->hair = HairData();
    c->hair.xyz.assign(xyz, xyz + 3 * n);
    c->hair.starts.assign(starts, starts + n);
    c->hair.starts.push_back(1);
    if (n) c->hair.starts[0] = 1;
    c->hair.radius = radius;
    c->hair.shapeRadius = {radius};
    c->hair.shapeFirst = {0};
    HairShapeDesc h;
    h.radius = radius;
    c->desc.shapes.assign(1, h);
    c->haveHair = true;
    c->prepared = false;
    return HPT_OK;
}

int hpt_set_bsdf_marschner(hpt_context *c, float int_ior, float ext_ior, int distribution, float alpha,
                           const float diffuse[3], const float specular[3]) {
    if (!c || distribution < 0 || distribution > 2 || !diffuse) return setErr(c, HPT_EINVAL, "bad marschner params");
    static const char *names[3] = {"beckmann", "ggx", "phong"};
    BsdfDesc &b = singleBsdf(c->desc, "marschner");
    b.intIOR = int_ior;
    b.extIOR = ext_ior;
    b.distribution = names[distribution];
    b.alpha = alpha;
    for (int i = 0; i < 3; ++i) {
        b.diffuse[i] = diffuse[i];
        b.specular[i] = specular ? specular[i] : 0.5f;
    }
    c->haveBSDF = true;
    c->prepared = false;
    return HPT_OK;
}

int hpt_set_bsdf_roughplastic(hpt_context *c, float int_ior, float ext_ior, int distribution, float alpha,
                              int sample_visible, int nonlinear, const float diffuse[3], const float specular[3]) {
    if (!c || distribution < 0 || distribution > 2) return setErr(c, HPT_EINVAL, "bad roughplastic params");
    if (int_ior < 0 || ext_ior < 0 || int_ior == ext_ior)
        return setErr(c, HPT_EINVAL, "The interior and exterior indices of refraction must be positive and differ!");
    static const char *names[3] = {"beckmann", "ggx", "phong"};
    BsdfDesc &b = singleBsdf(c->desc, "roughplastic");
    b.intIOR = int_ior;
    b.extIOR = ext_ior;
    b.distribution = names[distribution];
    b.alpha = alpha;
    b.sampleVisible = sample_visible != 0;
    b.nonlinear = nonlinear != 0;
    for (int i = 0; i < 3; ++i) {
        b.diffuse[i] = diffuse ? diffuse[i] : 0.5f;
        b.specular[i] = specular ? specular[i] : 1.0f;
    }
    c->haveBSDF = true;
    c->prepared = false;
    return HPT_OK;
}

int hpt_set_bsdf_marschnerdielectric(hpt_context *c, float int_ior, float ext_ior, const float diffuse[3],
                                     const float specular_reflectance[3], const float specular_transmittance[3]) {
    if (!c) return HPT_EINVAL;
    if (int_ior < 0 || ext_ior < 0)
        return setErr(c, HPT_EINVAL, "The interior and exterior indices of refraction must be positive!");
    BsdfDesc &b = singleBsdf(c->desc, "marschnerdielectric");
    b.intIOR = int_ior;
    b.extIOR = ext_ior;
    for (int i = 0; i < 3; ++i) {
        b.diffuse[i] = diffuse ? diffuse[i] : 0.5f;
        b.specular[i] = specular_reflectance ? specular_reflectance[i] : 0.1f;
        b.transmittance[i] = specular_transmittance ? specular_transmittance[i] : 0.1f;
    }
    c->haveBSDF = true;
    c->prepared = false;
    return HPT_OK;
}

int hpt_set_bsdf_kajiyakay(hpt_context *c, const float kd[3], const float ks[3], float exponent) {
    if (!c || !kd) return HPT_EINVAL;
    BsdfDesc &b = singleBsdf(c->desc, "kajiyakay");
    for (int i = 0; i < 3; ++i) {
        b.diffuse[i] = kd[i];
        b.specular[i] = ks ? ks[i] : 0.2f;
    }
    b.exponent = exponent;
    c->haveBSDF = true;
    c->prepared = false;
    return HPT_OK;
}

int hpt_set_envmap_rgb(hpt_context *c, const float *rgb, int w, int h, float scale, const float *to_world) {
    if (!c || !rgb || w <= 0 || h <= 0) return setErr(c, HPT_EINVAL, "bad envmap");
    c->env = EnvHost();
    c->env.w = w;
    c->env.h = h;
    c->env.rgb.assign(rgb, rgb + (size_t) w * h * 3);
    c->env.scale = scale;
    if (to_world) std::memcpy(c->env.toWorld, to_world, sizeof(c->env.toWorld));
    c->desc.emitter = "envmap";
    c->envFromSunsky = false;
    c->haveEnv = true;
    c->prepared = false;
    return HPT_OK;
}

int hpt_set_sunsky(hpt_context *c, const float sun_direction[3], float turbidity, float sky_scale, float sun_scale,
                   float sun_radius_scale, int resolution) {
    if (!c || !sun_direction || resolution < 4) return HPT_EINVAL;
    c->desc.emitter = "sunsky";
    for (int i = 0; i < 3; ++i) c->desc.sunDirection[i] = sun_direction[i];
    c->desc.turbidity = turbidity;
    c->desc.skyScale = sky_scale;
    c->desc.sunScale = sun_scale;
    c->desc.sunRadiusScale = sun_radius_scale;
    c->desc.skyResolution = resolution;
    c->desc.sunDirectionGiven = true;
    c->envFromSunsky = true;
    c->haveEnv = true;
    c->prepared = false;
    return HPT_OK;
}

static_assert(HPT_RFILTER_BOX == HPT_FILTER_BOX && HPT_RFILTER_TENT == HPT_FILTER_TENT &&
                  HPT_RFILTER_GAUSSIAN == HPT_FILTER_GAUSSIAN && HPT_RFILTER_MITCHELL == HPT_FILTER_MITCHELL &&
                  HPT_RFILTER_CATMULLROM == HPT_FILTER_CATMULLROM && HPT_RFILTER_LANCZOS == HPT_FILTER_LANCZOS,
              "hairpt.h numbers the filters like the host code");

int hpt_set_rfilter(hpt_context *c, int type, float p0, float p1) {
    if (!c) return HPT_EINVAL;
    float lut[HPT_FILTER_RES + 1], scale, radius;
    int border;
    std::string err;
    if (!setupFilter(type, p0, p1, lut, scale, radius, border, err)) return setErr(c, HPT_EINVAL, err);
    c->desc.rfilter = kFilterNames[type];
    c->desc.rfilterP0 = p0;
    c->desc.rfilterP1 = p1;
    /* the film filter is no part of what hpt_prepare builds (kd-tree, tables): a prepared
       context takes it at once; the next render uploads the changed scene record */
    if (c->prepared) return configureFilter(c);
    return HPT_OK;
}

int hpt_get_rfilter(hpt_context *c, int *type, float *radius, int *border, float lut[32], float *scale) {
    if (!c) return HPT_EINVAL;
    float l[HPT_FILTER_RES + 1], s, r;
    int b;
    std::string err;
    const int t = filterTypeOf(c->desc.rfilter);
    if (!setupFilter(t, c->desc.rfilterP0, c->desc.rfilterP1, l, s, r, b, err)) return setErr(c, HPT_EINVAL, err);
    static_assert(HPT_FILTER_RES + 1 == 32, "hairpt.h documents a 32-entry LUT");
    if (type) *type = t;
    if (radius) *radius = r;
    if (border) *border = b;
    if (lut) std::memcpy(lut, l, sizeof(l));
    if (scale) *scale = s;
    return HPT_OK;
}

static int uploadScene(hpt_context *c);

int hpt_prepare(hpt_context *c) {
    if (!c) return HPT_EINVAL;
    if (!c->haveCamera || !c->haveHair || !c->haveBSDF || !c->haveEnv)
        return setErr(c, HPT_ESTATE, "scene incomplete: need camera, hair, bsdf and emitter");
    if (!c->desc.meshes.empty() && !c->desc.shapes.empty())
        return setErr(c, HPT_EINVAL, "scene mixes hair with obj/rectangle shapes: the device path renders a hair "
                                     "scene or a triangle-mesh scene (C1), not both");
    c->prepared = false;
    c->meshScene = !c->desc.meshes.empty();
    const SceneDesc &d = c->desc;
    if (c->meshScene) {
        /* C1: the meshes, their BSDFs (diffuse / plastic / twosided) and the environment; the
           camera, sampler and film are the hair path's */
        try {
            if (c->sobol32.empty()) {
                std::string dir = c->dataDir + "/sobol/";
                if (!readFile(dir + "matrices32.u32", c->sobol32) || c->sobol32.size() != HPT_SOBOL_DIMS * HPT_SOBOL_BITS ||
                    !readFile(dir + "vdc.u64", c->vdc) || !readFile(dir + "vdc_inv.u64", c->vdcInv))
                    return setErr(c, HPT_EIO, "cannot read Sobol tables from " + dir);
            }
            if (d.emitter != "envmap" && d.emitter != "sunsky")
                return setErr(c, HPT_EINVAL, "mesh scene without an envmap / sunsky emitter");
            c->mesh = buildMeshScene(d);
            if (c->mesh.depth + 1 > HPT_MESH_STACK)
                return setErr(c, HPT_EINVAL, "mesh BVH deeper than the traversal stack");
            c->hair = HairData();
            c->tree = KDTreeHost();
            c->mar.clear();
            c->rp.clear();
            c->bsdfRec.clear();
            if (c->envFromSunsky) {
                if (c->sunsky.hosek.empty()) {
                    std::string err;
                    if (!loadSunSkyTables(c->dataDir, c->sunsky, err)) return setErr(c, HPT_EIO, err);
                }
                c->env = EnvHost();
                rasterizeSunSky(d, c->sunsky, c->env);
            }
            buildEnvMap(c->env);
            buildEnvMipmap(c->env);
        } catch (const std::exception &e) {
            return setErr(c, HPT_EINVAL, e.what());
        }
        c->sceneId = 0;
        const int rc = uploadScene(c);
        if (rc == HPT_OK) {
            static std::atomic<uint64_t> meshCounter{1ull << 62};
            c->sceneId = ++meshCounter;
        }
        return rc;
    }
    try {
        /* Sobol tables (data/sobol, extracted from src/samplers/sobolseq.cpp) */
        if (c->sobol32.empty()) {
            std::string dir = c->dataDir + "/sobol/";
            if (!readFile(dir + "matrices32.u32", c->sobol32) || c->sobol32.size() != HPT_SOBOL_DIMS * HPT_SOBOL_BITS ||
                !readFile(dir + "vdc.u64", c->vdc) || !readFile(dir + "vdc_inv.u64", c->vdcInv))
                return setErr(c, HPT_EIO, "cannot read Sobol tables from " + dir);
        }
        if (c->hairFromFile) {
            c->hair = HairData();
            c->hair.shapeRadius.clear();
            for (const HairShapeDesc &h : d.shapes)
                appendHair(c->hair, loadHair(h.file, h.radius, h.angleThreshold, h.reduction,
                                             h.hasToWorld ? h.toWorld : nullptr));
        }
        c->tree = buildHairKDTree(c->hair, d.kd);
        const size_t nb = d.bsdfs.size();
        c->mar.assign(nb, MarschnerHost());
        c->rp.assign(nb, RoughPlasticHost());
        c->bsdfRec.assign(nb, HptBsdf());
        for (size_t i = 0; i < nb; ++i) {
            const BsdfDesc &b = d.bsdfs[i];
            HptBsdf &rec = c->bsdfRec[i];
            std::memset(&rec, 0, sizeof(rec));
            rec.kind = bsdfKindOf(b.type);
            rec.smooth = 1;
            std::string err;
            switch (rec.kind) {
            case HPT_BSDF_MARSCHNER:
                if (!precomputeMarschner(b, c->dataDir, c->mar[i], err)) return setErr(c, HPT_EIO, err);
                break;
            case HPT_BSDF_KAJIYAKAY: configureKajiyaKay(b, rec.kk); break;
            case HPT_BSDF_ROUGHPLASTIC:
                if (!configureRoughPlastic(b, c->dataDir, c->rp[i], err)) return setErr(c, HPT_EINVAL, err);
                rec.rp = c->rp[i].p;
                break;
            case HPT_BSDF_MARSCHNERDIELECTRIC: configureMarschnerDielectric(b, rec.md); break;
            case HPT_BSDF_THINDIELECTRIC:
                configureThinDielectric(b, rec.md);
                rec.smooth = 0; /* EDeltaReflection | ENull only */
                break;
            case HPT_BSDF_DIFFUSE:
                configureDiffuse(b, rec.df);
                /* no component at all when the reflectance is 0 (diffuse.cpp:81-84) */
                rec.smooth = std::max(std::max(rec.df.refl[0], rec.df.refl[1]), rec.df.refl[2]) > 0 ? 1 : 0;
                break;
            default: return setErr(c, HPT_EINVAL, "unsupported bsdf " + b.type);
            }
        }
        if (d.shapes.empty() || nb == 0) return setErr(c, HPT_ESTATE, "no hair shape / bsdf");
        if (c->envFromSunsky) {
            if (c->sunsky.hosek.empty()) {
                std::string err;
                if (!loadSunSkyTables(c->dataDir, c->sunsky, err)) return setErr(c, HPT_EIO, err);
            }
            c->env = EnvHost();
            rasterizeSunSky(d, c->sunsky, c->env);
        }
        buildEnvMap(c->env);
        buildEnvMipmap(c->env);
    } catch (const std::exception &e) {
        return setErr(c, HPT_EIO, e.what());
    }
    c->sceneId = 0;
    const int rc = uploadScene(c);
    if (rc == HPT_OK) {
        static std::atomic<uint64_t> counter{0};
        c->sceneId = ++counter;
    }
    return rc;
}

/* the device half of hpt_prepare: the host-built scene (kd-tree, tables, envmap) to this
   context's device and the kernels' HptScene record.  hpt_context_share_scene runs it alone on a
   context that copied another's host scene */
static int uploadScene(hpt_context *c) {
    const SceneDesc &d = c->desc;
    if (c->device != HPT_HOST_ONLY) {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        freeBufs(c->sceneBufs);
    }
    HptScene &sc = c->sc;
    std::memset(&sc, 0, sizeof(sc));
    try {
        setupCamera(d, sc.cam);
    } catch (const std::exception &e) {
        return setErr(c, HPT_EINVAL, e.what());
    }
    int r = 0;
    r |= upload(c, c->tree.nodes.data(), c->tree.nodes.size() * sizeof(HptNode), (const void **) &sc.nodes);
    r |= upload(c, c->tree.nodes4.data(), c->tree.nodes4.size() * sizeof(HptNode4), (const void **) &sc.nodes4);
    r |= upload(c, c->tree.leafTable.data(), c->tree.leafTable.size() * 4, (const void **) &sc.leafTable);
    r |= upload(c, c->tree.leafF.data(), c->tree.leafF.size() * sizeof(HptSegF), (const void **) &sc.leafF);
    r |= upload(c, c->tree.leafQ.data(), c->tree.leafQ.size() * sizeof(HptSegQ), (const void **) &sc.leafQ);
    r |= upload(c, c->tree.prims.data(), c->tree.prims.size() * 4, (const void **) &sc.leafSeg);
    r |= upload(c, c->tree.segs.data(), c->tree.segs.size() * sizeof(HptSegment), (const void **) &sc.segs);
    for (int i = 0; i < 3; ++i) { /* the scene bounds: the hair kd-tree's, or the mesh scene's */
        sc.aabbMin[i] = c->meshScene ? c->mesh.aabbMin[i] : c->tree.aabbMin[i];
        sc.aabbMax[i] = c->meshScene ? c->mesh.aabbMax[i] : c->tree.aabbMax[i];
    }
    /* BSDF records: device tables first, then the records themselves */
    for (size_t i = 0; i < c->bsdfRec.size(); ++i) {
        HptBsdf &rec = c->bsdfRec[i];
        if (rec.kind == HPT_BSDF_MARSCHNER) {
            const MarschnerHost &m = c->mar[i];
            for (int l = 0; l < 3; ++l) {
                r |= upload(c, m.table[l].data(), m.table[l].size() * 16, (const void **) &rec.mar.table[l]);
                r |= upload(c, m.cdf[l].data(), m.cdf[l].size() * 4, (const void **) &rec.mar.cdf[l]);
                r |= upload(c, m.sums[l].data(), m.sums[l].size() * 4, (const void **) &rec.mar.sums[l]);
            }
            r |= upload(c, m.trans.data(), m.trans.size() * 4, (const void **) &rec.mar.trans);
            rec.mar.transSize = (int) m.trans.size();
            rec.mar.fdr = m.fdr;
            rec.mar.invEta2 = m.invEta2;
            rec.mar.specularSamplingWeight = m.specularSamplingWeight;
            rec.mar.vR = m.vR;
            rec.mar.vTT = m.vTT;
            rec.mar.vTRT = m.vTRT;
            rec.mar.scaleAngleRad = m.scaleAngleRad;
            const float lobeV[3] = {m.vR, m.vTT, m.vTRT};
            for (int l = 0; l < 3; ++l) {
                const float v = lobeV[l];
                rec.mar.lobeInvV[l] = 1.0f / v;
                rec.mar.lobeK[l] = v < 0.1f ? logf(1.0f / (2.0f * v)) : 2.0f * v * sinhf(1.0f / v);
            }
            for (int k = 0; k < 3; ++k) rec.mar.diffuse[k] = m.diffuse[k];
        } else if (rec.kind == HPT_BSDF_ROUGHPLASTIC) {
            r |= upload(c, c->rp[i].trans.data(), c->rp[i].trans.size() * 4, (const void **) &rec.rp.trans);
        }
    }
    const size_t nShapes = std::max<size_t>(1, c->hair.shapeRadius.size());
    if (nShapes > HPT_MAX_SHAPES) return setErr(c, HPT_EINVAL, "too many hair shapes");
    std::vector<HptShape> shapes(nShapes);
    for (size_t k = 0; k < nShapes; ++k) {
        shapes[k].radius = c->hair.shapeRadius.empty() ? c->hair.radius : c->hair.shapeRadius[k];
        shapes[k].bsdf = k < d.shapes.size() ? d.shapes[k].bsdf : 0;
    }
    sc.nShapes = (int) nShapes;
    sc.radius = shapes[0].radius;
    sc.maxRadius = 0.0f;
    for (const HptShape &h : shapes) sc.maxRadius = std::max(sc.maxRadius, h.radius);
    sc.preRadius = c->tree.preRadius;
    if (!c->bsdfRec.empty()) sc.bsdf = c->bsdfRec[shapes[0].bsdf];
    if (nShapes > 1) {
        r |= upload(c, shapes.data(), shapes.size() * sizeof(HptShape), (const void **) &sc.shapes);
        r |= upload(c, c->bsdfRec.data(), c->bsdfRec.size() * sizeof(HptBsdf), (const void **) &sc.bsdfs);
    }
    /* environment (envmap.cpp) + scene bounding sphere (scene.cpp:386-412, envmap.cpp:336-347) */
    HptEnvMap &E = sc.env;
    r |= upload(c, c->env.texel.data(), c->env.texel.size() * 16, (const void **) &E.texel);
    r |= upload(c, c->env.cdfRows.data(), c->env.cdfRows.size() * 4, (const void **) &E.cdfRows);
    r |= upload(c, c->env.cdfCols.data(), c->env.cdfCols.size() * 4, (const void **) &E.cdfCols);
    r |= upload(c, c->env.rowWeights.data(), c->env.rowWeights.size() * 4, (const void **) &E.rowWeights);
    r |= upload(c, c->env.guideRows.data(), c->env.guideRows.size() * 4, (const void **) &E.guideRows);
    r |= upload(c, c->env.guideCols.data(), c->env.guideCols.size() * 4, (const void **) &E.guideCols);
    {
        std::vector<HptMipLevel> lv(c->env.levelW.size());
        for (size_t l = 0; l < lv.size(); ++l)
            lv[l] = {c->env.levelW[l], c->env.levelH[l], c->env.levelOff[l], c->env.ratioX[l], c->env.ratioY[l]};
        r |= upload(c, c->env.mip.data(), c->env.mip.size() * 16, (const void **) &E.mip);
        r |= upload(c, lv.data(), lv.size() * sizeof(HptMipLevel), (const void **) &E.levels);
        r |= upload(c, c->env.ewaLut, sizeof(c->env.ewaLut), (const void **) &E.ewaLut);
        E.nLevels = (int) lv.size();
        E.maxAnisotropy = 10.0f; /* envmap.cpp:142 */
    }
    E.w = c->env.w;
    E.h = c->env.h;
    E.normalization = c->env.normalization;
    E.scale = c->env.scale;
    E.pixelSizeX = c->env.pixelSizeX;
    E.pixelSizeY = c->env.pixelSizeY;
    E.identity = 1;
    for (int i = 0; i < 16; ++i) E.identity &= c->env.toWorld[i] == ((i % 5 == 0) ? 1.0f : 0.0f);
    if (!E.identity) {
        double m[9], inv[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                E.m[i * 3 + j] = c->env.toWorld[i * 4 + j];
                m[i * 3 + j] = c->env.toWorld[i * 4 + j];
            }
        double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) +
                     m[2] * (m[3] * m[7] - m[4] * m[6]);
        inv[0] = (m[4] * m[8] - m[5] * m[7]) / det;
        inv[1] = (m[2] * m[7] - m[1] * m[8]) / det;
        inv[2] = (m[1] * m[5] - m[2] * m[4]) / det;
        inv[3] = (m[5] * m[6] - m[3] * m[8]) / det;
        inv[4] = (m[0] * m[8] - m[2] * m[6]) / det;
        inv[5] = (m[2] * m[3] - m[0] * m[5]) / det;
        inv[6] = (m[3] * m[7] - m[4] * m[6]) / det;
        inv[7] = (m[1] * m[6] - m[0] * m[7]) / det;
        inv[8] = (m[0] * m[4] - m[1] * m[3]) / det;
        for (int i = 0; i < 9; ++i) E.minv[i] = (float) inv[i];
    }
    {
        float mn[3], mx[3];
        for (int i = 0; i < 3; ++i) {
            mn[i] = sc.aabbMin[i];
            mx[i] = sc.aabbMax[i];
        }
        float cam[3] = {d.toWorld[3], d.toWorld[7], d.toWorld[11]};
        for (int i = 0; i < 3; ++i) {
            mn[i] = std::min(mn[i], cam[i]);
            mx[i] = std::max(mx[i], cam[i]);
        }
        float ctr[3], dd[3];
        for (int i = 0; i < 3; ++i) {
            ctr[i] = (mx[i] + mn[i]) * 0.5f;
            dd[i] = ctr[i] - mx[i];
        }
        float radius = std::sqrt(dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]);
        for (int i = 0; i < 3; ++i) E.bsCenter[i] = ctr[i];
        E.bsRadius = std::max(1e-4f, radius * 1.5f);
    }
    if (c->meshScene) { /* the mesh scene's arrays (HptMeshScene) */
        const MeshSceneHost &M = c->mesh;
        HptMeshScene &ms = c->ms;
        std::memset(&ms, 0, sizeof(ms));
        r |= upload(c, M.nodes.data(), M.nodes.size() * sizeof(HptBvhNode), (const void **) &ms.nodes);
        r |= upload(c, M.prims.data(), M.prims.size() * 4, (const void **) &ms.prims);
        r |= upload(c, M.tris.data(), M.tris.size() * sizeof(HptTri), (const void **) &ms.tris);
        r |= upload(c, M.rects.data(), M.rects.size() * sizeof(HptRect), (const void **) &ms.rects);
        r |= upload(c, M.meshes.data(), M.meshes.size() * sizeof(HptMeshInfo), (const void **) &ms.meshes);
        r |= upload(c, M.p.data(), M.p.size() * 4, (const void **) &ms.p);
        r |= upload(c, M.n.data(), M.n.size() * 4, (const void **) &ms.n);
        r |= upload(c, M.uv.data(), M.uv.size() * 4, (const void **) &ms.uv);
        r |= upload(c, M.dpdu.data(), M.dpdu.size() * 4, (const void **) &ms.dpdu);
        r |= upload(c, M.bsdfs.data(), M.bsdfs.size() * sizeof(HptMeshBsdf), (const void **) &ms.bsdfs);
        for (int i = 0; i < 3; ++i) ms.aabbMin[i] = M.aabbMin[i], ms.aabbMax[i] = M.aabbMax[i];
        ms.nNodes = (uint32_t) M.nodes.size();
        ms.stackDepth = M.depth + 1;
    }
    r |= upload(c, c->sobol32.data(), c->sobol32.size() * 4, (const void **) &sc.sobol);
    sc.scramble = 0;
    if (d.scramble) { /* sobol.cpp:96-102: sampleTEA of the two 32-bit halves (qmc.h:146-156) */
        uint32_t v0 = (uint32_t) d.scramble, v1 = (uint32_t) (d.scramble >> 32), sum = 0;
        for (int i = 0; i < 4; ++i) {
            sum += 0x9e3779b9u;
            v0 += ((v1 << 4) + 0xA341316Cu) ^ (v1 + sum) ^ ((v1 >> 5) + 0xC8013EA4u);
            v1 += ((v0 << 4) + 0xAD90777Du) ^ (v0 + sum) ^ ((v0 >> 5) + 0x7E95761Eu);
        }
        sc.scramble = v0; /* sampleSingle / look_up use the low 32 bits */
    }
    r |= upload(c, c->vdc.data(), c->vdc.size() * 8, (const void **) &sc.vdc);
    r |= upload(c, c->vdcInv.data(), c->vdcInv.size() * 8, (const void **) &sc.vdcInv);
    {
        static const uint32_t zero[4] = {0, 0, 0, 0};
        r |= upload(c, zero, sizeof(zero), (const void **) &sc.fault);
    }
    if (r) return HPT_EDEVICE;
    if (int rf = configureFilter(c)) return rf;
    c->samplesSpp = 0;
    sc.maxDepth = d.maxDepth;
    sc.rrDepth = d.rrDepth;
    sc.strictNormals = d.strictNormals ? 1 : 0;
    sc.hideEmitters = d.hideEmitters ? 1 : 0;
    if (sc.cam.logRes > (uint32_t) c->vdc.size() / HPT_SOBOL_BITS)
        return setErr(c, HPT_EINVAL, "image resolution exceeds the Sobol look-up tables");
    c->sc.maxLeafRounds = c->maxLeafRounds;
    c->sc.maxRestarts = c->maxRestarts;
    c->sc.packetStack = c->packetStack;
    c->schedules.clear();
    c->prepared = true;
    return HPT_OK;
}

int hpt_get_film_params(hpt_context *c, hpt_film_params *o) {
    if (!c || !o) return HPT_EINVAL;
    const FilmDesc &f = c->desc.film;
    std::memset(o, 0, sizeof(*o));
    o->ldr = f.type == "ldrfilm";
    o->file_format = o->ldr ? HPT_FILE_PNG
                     : f.fileFormat == "rgbe" ? HPT_FILE_RGBE
                     : f.fileFormat == "pfm"  ? HPT_FILE_PFM
                                              : HPT_FILE_OPENEXR;
    o->luminance = f.pixelFormat == "luminance";
    o->component_format = f.componentFormat == "float32" ? HPT_COMPONENT_FLOAT32
                          : f.componentFormat == "uint32" ? HPT_COMPONENT_UINT32
                                                          : HPT_COMPONENT_FLOAT16;
    o->reinhard = f.tonemapMethod == "reinhard";
    o->gamma = f.gamma;
    o->exposure = f.exposure;
    o->key = f.key;
    o->burn = f.burn;
    o->banner = f.banner;
    return HPT_OK;
}

int hpt_write_film(hpt_context *c, const char *path, const float *rgbw, int w, int h, const hpt_film_params *p,
                   char *written, int cap) {
    if (!c || !path || !rgbw || !p || w <= 0 || h <= 0) return setErr(c, HPT_EINVAL, "bad film arguments");
    FilmDesc f;
    f.type = p->ldr ? "ldrfilm" : "hdrfilm";
    static const char *files[4] = {"png", "openexr", "rgbe", "pfm"};
    static const char *comps[3] = {"float16", "float32", "uint32"};
    if (p->file_format < 0 || p->file_format > 3 || p->component_format < 0 || p->component_format > 2)
        return setErr(c, HPT_EINVAL, "bad film format");
    f.fileFormat = files[p->file_format];
    f.pixelFormat = p->luminance ? "luminance" : "rgb";
    f.componentFormat = comps[p->component_format];
    f.tonemapMethod = p->reinhard ? "reinhard" : "gamma";
    f.gamma = p->gamma;
    f.exposure = p->exposure;
    f.key = p->key;
    f.burn = p->burn;
    f.banner = p->banner != 0;
    std::string err, out;
    FilmImage img;
    if (!checkFilm(f, err) || !developFilm(rgbw, w, h, f, c->dataDir, img, err) || !writeFilm(path, img, f, out, err))
        return setErr(c, HPT_EIO, err);
    if (written && cap > 0) {
        std::strncpy(written, out.c_str(), (size_t) cap - 1);
        written[cap - 1] = 0;
    }
    return HPT_OK;
}

int hpt_get_scene_info(hpt_context *c, hpt_scene_info *o) {
    if (!c || !o) return HPT_EINVAL;
    std::memset(o, 0, sizeof(*o));
    const SceneDesc &d = c->desc;
    o->width = d.width;
    o->height = d.height;
    o->spp = d.spp;
    o->max_depth = d.maxDepth;
    o->rr_depth = d.rrDepth;
    o->strict_normals = d.strictNormals;
    o->hide_emitters = d.hideEmitters;
    o->bsdf = d.bsdfs.empty() ? -1 : bsdfKindOf(d.bsdfs[d.shapes.empty() ? 0 : d.shapes[0].bsdf].type);
    o->n_shapes = (int) std::max<size_t>(1, c->hair.shapeRadius.size());
    o->vertices = c->hair.vertexCount();
    o->segments = c->tree.segs.size();
    o->kd_nodes = c->tree.nodes.size();
    o->kd_indices = c->tree.prims.size();
    o->kd_depth = c->tree.maxDepthUsed;
    o->kd_build_seconds = c->tree.buildSeconds;
    for (int i = 0; i < 3; ++i) {
        o->aabb_min[i] = c->tree.aabbMin[i];
        o->aabb_max[i] = c->tree.aabbMax[i];
        o->bsphere_center[i] = c->sc.env.bsCenter[i];
    }
    o->bsphere_radius = c->sc.env.bsRadius;
    if (c->meshScene) { /* a mesh scene: its BVH in the kd fields, its bounds */
        o->kd_nodes = c->mesh.nodes.size();
        o->kd_indices = c->mesh.prims.size();
        o->kd_depth = (int) c->mesh.depth;
        o->vertices = c->mesh.vertexCount();
        for (int i = 0; i < 3; ++i) o->aabb_min[i] = c->mesh.aabbMin[i], o->aabb_max[i] = c->mesh.aabbMax[i];
    }
    return HPT_OK;
}

int hpt_context_share_scene(hpt_context *src, int device, hpt_context **out) {
    tlsErr.clear(); /* hpt_last_error(NULL) describes this call only */
    if (!src || !out) return HPT_EINVAL;
    *out = nullptr;
    /* src is only read here (several threads may share one source at once): failures are
       reported to the calling thread, hpt_last_error(NULL), never written to src */
    if (!src->prepared) return setErr(nullptr, HPT_ESTATE, "hpt_context_share_scene: the source context is not prepared");
    hpt_context *c = nullptr;
    int rc = hpt_context_create(device, &c);
    if (rc)
        return setErr(nullptr, rc, "hpt_context_share_scene: no gfx950 context on device " + std::to_string(device));
    /* the host-built scene, as hpt_prepare left it on src */
    c->dataDir = src->dataDir;
    c->desc = src->desc;
    c->haveCamera = src->haveCamera, c->haveHair = src->haveHair, c->haveBSDF = src->haveBSDF;
    c->haveEnv = src->haveEnv, c->hairFromFile = src->hairFromFile, c->envFromSunsky = src->envFromSunsky;
    c->hair = src->hair;
    c->tree = src->tree;
    c->meshScene = src->meshScene;
    c->mesh = src->mesh;
    c->mar = src->mar;
    c->rp = src->rp;
    c->bsdfRec = src->bsdfRec;
    c->env = src->env;
    c->sobol32 = src->sobol32;
    c->vdc = src->vdc;
    c->vdcInv = src->vdcInv;
    c->maxLeafRounds = src->maxLeafRounds, c->maxRestarts = src->maxRestarts, c->packetStack = src->packetStack;
    c->tailPaths = src->tailPaths, c->bounceAhead = src->bounceAhead, c->packets = src->packets;
    /* the shard deal: hpt_render_multi gives shard g to context g, and every context must deal
       the blocks the same way or some blocks are rendered twice and others never */
    c->blockWeights = src->blockWeights;
    c->weightsVersion = src->weightsVersion + 1;
    rc = uploadScene(c);
    if (rc) {
        setErr(nullptr, rc, c->err);
        hpt_context_destroy(c);
        return rc;
    }
    c->sceneId = src->sceneId;
    *out = c;
    return HPT_OK;
}

int64_t hpt_get_hair(hpt_context *c, float *xyz, uint8_t *starts) {
    if (!c) return HPT_EINVAL;
    int64_t n = (int64_t) c->hair.vertexCount();
    if (xyz) std::memcpy(xyz, c->hair.xyz.data(), (size_t) n * 12);
    if (starts) std::memcpy(starts, c->hair.starts.data(), c->hair.starts.size());
    return n;
}

int hpt_get_kdtree(hpt_context *c, uint32_t *nodes, int64_t *n_nodes, uint32_t *indices, int64_t *n_indices,
                   float aabb[6]) {
    if (!c || !n_nodes || !n_indices) return HPT_EINVAL;
    *n_nodes = (int64_t) c->tree.nodes.size();
    *n_indices = (int64_t) c->tree.prims.size();
    if (nodes) std::memcpy(nodes, c->tree.nodes.data(), c->tree.nodes.size() * 8);
    if (indices)
        for (size_t i = 0; i < c->tree.prims.size(); ++i) indices[i] = c->tree.segFirstVertex[c->tree.prims[i]];
    if (aabb)
        for (int i = 0; i < 3; ++i) {
            aabb[i] = c->tree.aabbMin[i];
            aabb[3 + i] = c->tree.aabbMax[i];
        }
    return HPT_OK;
}

int hpt_get_pretest_records(hpt_context *c, uint32_t *records, int64_t *n_records, float *radius,
                            uint64_t *n_pass) {
    if (!c || !n_records) return HPT_EINVAL;
    static_assert(sizeof(HptSegQ) == 16, "hairpt.h documents 16-byte records");
    const size_t n = c->tree.leafQ.size();
    *n_records = (int64_t) n;
    if (records) std::memcpy(records, c->tree.leafQ.data(), n * sizeof(HptSegQ));
    if (radius) *radius = c->tree.preRadius;
    if (n_pass) *n_pass = c->tree.prePassRecords;
    return HPT_OK;
}

int hpt_get_envmap(hpt_context *c, float *rgb, int *w, int *h) {
    if (!c || !w || !h) return HPT_EINVAL;
    *w = c->env.w;
    *h = c->env.h;
    if (rgb) std::memcpy(rgb, c->env.rgb.data(), c->env.rgb.size() * 4);
    return HPT_OK;
}

int hpt_get_camera(hpt_context *c, float s2c[16], float dx[3], float dy[3]) {
    if (!c || !s2c || !dx || !dy) return HPT_EINVAL;
    if (!c->haveCamera) return setErr(c, HPT_ESTATE, "no camera");
    HptCamera cam;
    try {
        setupCamera(c->desc, cam);
    } catch (const std::exception &e) {
        return setErr(c, HPT_EINVAL, e.what());
    }
    std::memcpy(s2c, cam.s2c, sizeof(cam.s2c));
    std::memcpy(dx, cam.dx, sizeof(cam.dx));
    std::memcpy(dy, cam.dy, sizeof(cam.dy));
    return HPT_OK;
}

int hpt_get_marschner_tables(hpt_context *c, float *nR, float *nTT, float *nTRT, float *fdr, float *trans,
                             float *specw) {
    if (!c || !c->prepared || c->sc.bsdf.kind != HPT_BSDF_MARSCHNER)
        return setErr(c, HPT_ESTATE, "no marschner bsdf prepared");
    const MarschnerHost &m = c->mar[c->desc.shapes.empty() ? 0 : c->desc.shapes[0].bsdf];
    float *outs[3] = {nR, nTT, nTRT};
    for (int l = 0; l < 3; ++l)
        if (outs[l])
            for (size_t i = 0; i < m.table[l].size(); ++i) {
                outs[l][3 * i] = m.table[l][i].x;
                outs[l][3 * i + 1] = m.table[l][i].y;
                outs[l][3 * i + 2] = m.table[l][i].z;
            }
    if (fdr) *fdr = m.fdr;
    if (trans) std::memcpy(trans, m.trans.data(), std::min<size_t>(100, m.trans.size()) * 4);
    if (specw) *specw = m.specularSamplingWeight;
    return HPT_OK;
}

int hpt_get_roughplastic_params(hpt_context *c, float *params, float *trans, int *trans_size) {
    if (!c || !c->prepared || c->sc.bsdf.kind != HPT_BSDF_ROUGHPLASTIC || c->rp.empty())
        return setErr(c, HPT_ESTATE, "no roughplastic bsdf prepared");
    const RoughPlasticHost &h = c->rp[c->desc.shapes.empty() ? 0 : c->desc.shapes[0].bsdf];
    const HptRoughPlastic &p = h.p;
    if (params) {
        const float v[16] = {(float) p.type, (float) p.sampleVisible, (float) p.nonlinear, p.alpha, p.exponent, p.eta,
                             p.invEta2, p.specularSamplingWeight, p.diffuse[0], p.diffuse[1], p.diffuse[2],
                             p.specular[0], p.specular[1], p.specular[2], p.fdr, (float) h.trans.size()};
        std::memcpy(params, v, sizeof(v));
    }
    if (trans_size) *trans_size = (int) h.trans.size();
    if (trans) std::memcpy(trans, h.trans.data(), h.trans.size() * 4);
    return HPT_OK;
}

} /* extern "C" */
