/*
 * hpt_context.h -- struct hpt_context and the helpers the files of the C ABI share
 * (hpt_capi.cpp, hpt_render_driver.cpp, hpt_render_multi.cpp, hpt_capi_batch.cpp).
 * Private to csrc/: not installed, not included from include/.
 */
#ifndef HPT_CONTEXT_H
#define HPT_CONTEXT_H
#include <hip/hip_runtime.h>

#include <array>
#include <map>
#include <string>
#include <vector>

#include "../../include/hairpt.h"
#include "../../include/hairpt_test.h"
#include "host/host_scene.h"
#include "hpt_device.h"
#include "kernels/hpt_kernels.h"

using namespace hpt;

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

/* the bounce schedule of a wave of paths: the shade-queue length of each wavefront bounce,
   and whether a k_tail launch took the rest */
struct BounceSchedule {
    std::vector<uint32_t> shade;
    bool tail = false;
};

/* what the files share is no part of the library's interface: hidden from its symbol table */
#pragma GCC visibility push(hidden)
/* hpt_capi.cpp: the environment's defaults of a new context */
uint32_t defaultTailPaths();
bool defaultPackets();
bool defaultBounceAhead();
int scheduleTestHook();
int setErr(hpt_context *c, int code, const std::string &m);
int upload(hpt_context *c, const void *src, size_t bytes, const void **dst);
void freeBufs(std::vector<DevBuf> &v);
int clearFault(hpt_context *c);
int checkFault(hpt_context *c);
hipEvent_t takeEvent(hpt_context *c, size_t &used);
/* hpt_render_driver.cpp: the wavefront driver (hpt_render, hpt_render_device, hpt_render_multi) */
int renderImpl(hpt_context *c, const hpt_render_params *prm, float4 *dFilm);
#pragma GCC visibility pop

#define HIPCHK(ctx, expr)                                                                                   \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess)                                                                               \
            return setErr(ctx, HPT_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));            \
    } while (0)

struct hpt_context {
    int device = 0;
    uint32_t tailPaths = defaultTailPaths();
    bool bounceAhead = defaultBounceAhead();
    int scheduleTest = scheduleTestHook();
    /* schedules of the waves rendered since the last prepare, by (spp begin, spp count,
       shard, shards): a repeated wave launches its bounces ahead on that schedule */
    std::map<std::array<int64_t, 4>, BounceSchedule> schedules;
    uint32_t maxLeafRounds = HPT_MAX_LEAF_ROUNDS, maxRestarts = HPT_MAX_RESTARTS; /* traversal bounds */
    uint32_t packetStack = 0;      /* 0 = the kernel's packet stack depth */
    bool packets = defaultPackets();
    hipStream_t stream = nullptr;
    uint32_t *hostCnt = nullptr; /* pinned copy of the counter block */
    std::vector<uint8_t> scShadow; /* the HptScene last copied to scDev */
    std::string err;
    std::string dataDir;
    SceneDesc desc;
    bool haveCamera = false, haveHair = false, haveBSDF = false, haveEnv = false, prepared = false;
    bool hairFromFile = false;     /* desc.shapes are loaded from files at prepare */
    HairData hair;                 /* every hair shape, merged */
    KDTreeHost tree;
    /* a triangle-mesh scene (C1: obj / rectangle shapes, no hair): mesh.cpp's arrays and their
       device view; k_mesh_paths renders it */
    bool meshScene = false;
    MeshSceneHost mesh;
    HptMeshScene ms{};
    /* per BSDF of desc.bsdfs: host tables and the device record */
    std::vector<MarschnerHost> mar;
    std::vector<RoughPlasticHost> rp;
    std::vector<HptBsdf> bsdfRec;
    EnvHost env;
    bool envFromSunsky = false;
    SunSkyTables sunsky;
    std::vector<uint32_t> sobol32;
    std::vector<uint64_t> vdc, vdcInv;
    HptScene sc;
    HptScene *scDev = nullptr;     /* device copy of sc (kernels that read the scene through a pointer) */
    std::vector<DevBuf> sceneBufs;
    /* wave buffers */
    uint64_t capacity = 0;
    std::vector<DevBuf> waveBufs;
    HptPaths P;
    /* rays of the bounce; paths to shade by bounce parity (shadeQ[p] is post's output for p ^ 1) */
    uint32_t *qTrace = nullptr, *qShadow = nullptr, *qShade[2] = {nullptr, nullptr};
    uint32_t *counters = nullptr;
    uint64_t *dstats = nullptr;
    float4 *partial = nullptr;     /* film splat partials: slots x (2 border + 1)^2 (k_splat -> k_gather) */
    uint64_t partialCap = 0;       /* float4s allocated */
    /* the last hpt_render's samples are still in P.pos / P.li, in its shard's slot order, when it
       was one wave of this many samples per pixel (hpt_get_render_samples); 0: not available */
    uint32_t samplesSpp = 0;
    /* block ownership of the last render call's shard (blockOf / localOf of HptWave) */
    uint32_t *dBlockOf = nullptr;
    int32_t *dLocalOf = nullptr;
    int ownW = -1, ownH = -1, ownShard = -1, ownShards = -1, ownCap = 0, ownLocal = 0;
    uint64_t ownWeights = 0;            /* weightsVersion the ownership tables were dealt with */
    std::vector<uint32_t> ownBlocks;    /* the image blocks of dBlockOf, on the host */
    uint32_t *dBlockCost = nullptr;     /* path-bounces shaded per owned block (HptPaths::blockCost) */
    std::vector<double> blockWeights;   /* hpt_set_block_weights (empty: Hilbert-cyclic deal) */
    uint64_t weightsVersion = 0;
    /* the prepared scene this context renders: a process-unique number given by each successful
       hpt_prepare and copied by hpt_context_share_scene, so hpt_render_multi can refuse contexts
       that would render different scenes into one film (0: not prepared) */
    uint64_t sceneId = 0;
    hpt_stats stats;
    std::vector<hipEvent_t> evPool;
    /* hpt_render_multi: this context's shard film, and (on the receiving context) the staging
       buffer the other devices' films are copied into */
    float4 *mfilm = nullptr, *mstage = nullptr;
    size_t mfilmPixels = 0, mstagePixels = 0;
    std::vector<hipStream_t> peerStreams; /* one copy stream (and its done event) per peer film */
    std::vector<hipEvent_t> peerEvents;
};

#endif
