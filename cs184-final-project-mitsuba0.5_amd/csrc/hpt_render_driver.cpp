/*
 * hpt_render_driver.cpp -- the wavefront driver behind hpt_render, and the block-ownership
 * deal of its shards.
 *
 * The driver replaces SamplingIntegrator::render / BlockedRenderProcess
 * (src/librender/integrator.cpp:95-188, renderproc.cpp:26-145): instead of
 * one CPU worker per 32x32 block it runs every sample of every owned block
 * as one lane of a wave of paths resident in HBM, bouncing the whole wave
 * through k_shade -> k_trace -> k_post until its queue drains, then gathers
 * the wave into the film.  Waves are sized to HBM (hundreds of bytes per
 * path), so a 512x512x256 frame is a single wave on MI355X.
 */
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hpt_context.h"

namespace {

int ensureWave(hpt_context *c, uint64_t n) {
    if (n <= c->capacity) return HPT_OK;
    freeBufs(c->waveBufs);
    c->capacity = 0;
    auto alloc = [&](size_t bytes, void **p) -> int {
        DevBuf b;
        b.bytes = bytes;
        HIPCHK(c, hipMalloc(&b.p, bytes));
        c->waveBufs.push_back(b);
        *p = b.p;
        return HPT_OK;
    };
    int r = 0;
    r |= alloc(n * 16, (void **) &c->P.ro);
    r |= alloc(n * 16, (void **) &c->P.rd);
    r |= alloc(n * 8, (void **) &c->P.pos);
    r |= alloc(n * 8, (void **) &c->P.sobol);
    r |= alloc(n * 4, (void **) &c->P.state);
    r |= alloc(n * 16, (void **) &c->P.thr);
    r |= alloc(n * 16, (void **) &c->P.li);
    r |= alloc(n * 4, (void **) &c->P.hit);
    r |= alloc(n * 4, (void **) &c->P.hitQ);
    r |= alloc(n * 4, (void **) &c->P.hitS);
    r |= alloc(n * 64, (void **) &c->P.postRec);
    r |= alloc(n * 48, (void **) &c->P.shadowRec);
    r |= alloc(n * 48, (void **) &c->P.shadeRec);
    r |= alloc(n * 16, (void **) &c->P.bw);
    r |= alloc(n * 16, (void **) &c->P.sdir);
    r |= alloc(n * 16, (void **) &c->P.scontrib);
    r |= alloc(n * 4, (void **) &c->qTrace);
    r |= alloc(n * 4, (void **) &c->qShadow);
    r |= alloc(n * 4, (void **) &c->qShade[0]);
    r |= alloc(n * 4, (void **) &c->qShade[1]);
    r |= alloc(HPT_COUNTER_WORDS * 4, (void **) &c->counters);
    r |= alloc(2 * HPT_TS_COUNT * 8, (void **) &c->dstats); /* the counters, and a snapshot at the start of a wave */
    if (r) return HPT_EDEVICE;
    c->capacity = n;
    return HPT_OK;
}

/* the film splat's scratch: (2 border + 1)^2 partial sums per owned pixel slot */
int ensurePartial(hpt_context *c, uint64_t slots) {
    const uint64_t n = 2 * (uint64_t) c->sc.filterBorder + 1, need = slots * n * n;
    if (need <= c->partialCap) return HPT_OK;
    if (c->partial) (void) hipFree(c->partial);
    c->partial = nullptr;
    c->partialCap = 0;
    HIPCHK(c, hipMalloc((void **) &c->partial, need * sizeof(float4)));
    c->partialCap = need;
    return HPT_OK;
}

/* samples of every pixel per wave: the whole range, or as many as max_wave_paths (0 = automatic,
   HBM-sized waves) leaves room for over the shard's pixel slots */
uint32_t waveSpp(uint64_t slots, uint64_t sppCount, uint64_t maxWavePaths) {
    const uint64_t maxWave = maxWavePaths ? maxWavePaths : (uint64_t) 1 << 26;
    return (uint32_t) std::max<uint64_t>(1, std::min<uint64_t>(sppCount, maxWave / slots));
}

/* Image blocks in Hilbert-curve order over the nbx x nby grid of 32x32
   blocks.  Shard r of N owns every N-th block of this order (r, r+N, ...):
   N consecutive blocks of the curve are a compact patch of the image, so
   every shard gets one block of every patch and the hair's uneven screen
   coverage spreads evenly over the ranks (a plain b mod N deal gives
   whole block columns to a rank whenever N divides nbx). */
std::vector<uint32_t> blockOrder(int nbx, int nby) {
    uint32_t n = 1;
    while (n < (uint32_t) std::max(nbx, nby)) n <<= 1;
    std::vector<uint32_t> order;
    order.reserve((size_t) nbx * nby);
    for (uint64_t d = 0; d < (uint64_t) n * n; ++d) {
        uint32_t x = 0, y = 0;
        uint64_t t = d;
        for (uint32_t sq = 1; sq < n; sq <<= 1) { /* Hilbert index -> (x, y) */
            const uint32_t rx = 1u & (uint32_t) (t / 2), ry = 1u & (uint32_t) (t ^ rx);
            if (ry == 0) {
                if (rx == 1) {
                    x = sq - 1 - x;
                    y = sq - 1 - y;
                }
                std::swap(x, y);
            }
            x += sq * rx;
            y += sq * ry;
            t /= 4;
        }
        if ((int) x < nbx && (int) y < nby) order.push_back(y * (uint32_t) nbx + x);
    }
    return order;
}

/* The shard of every image block.  Without weights: position i of the Hilbert order goes to
   shard i mod N (compact patches of N blocks, one block each).  With weights (the measured
   work of each block, hpt_set_block_weights): longest-processing-time first -- blocks in
   descending weight (ties in Hilbert order) each to the shard with the least weight so far
   (ties to the lowest shard) -- the same deal on every rank given the same weights. */
std::vector<int> dealBlocks(int nbx, int nby, int nShards, const std::vector<double> &weights) {
    const std::vector<uint32_t> order = blockOrder(nbx, nby);
    std::vector<int> shardOf(order.size(), 0);
    if (weights.size() != order.size()) {
        for (size_t i = 0; i < order.size(); ++i) shardOf[order[i]] = (int) (i % (size_t) nShards);
        return shardOf;
    }
    std::vector<size_t> byWeight(order.size());
    for (size_t i = 0; i < order.size(); ++i) byWeight[i] = i; /* Hilbert positions */
    std::stable_sort(byWeight.begin(), byWeight.end(),
                     [&](size_t a, size_t b) { return weights[order[a]] > weights[order[b]]; });
    std::vector<double> load((size_t) nShards, 0.0);
    for (size_t k : byWeight) {
        const int r = (int) (std::min_element(load.begin(), load.end()) - load.begin());
        shardOf[order[k]] = r;
        load[(size_t) r] += weights[order[k]];
    }
    return shardOf;
}

/* upload this shard's block ownership tables (cached per frame shape, shard and deal) */
int ensureOwnership(hpt_context *c, int W, int H, int nbx, int nby, int shard, int nShards) {
    if (c->ownW == W && c->ownH == H && c->ownShard == shard && c->ownShards == nShards &&
        c->ownWeights == c->weightsVersion)
        return HPT_OK;
    if (!c->blockWeights.empty() && c->blockWeights.size() != (size_t) nbx * nby)
        return setErr(c, HPT_EINVAL, "hpt_set_block_weights gave " + std::to_string(c->blockWeights.size()) +
                                         " block weights for a frame of " + std::to_string(nbx * nby) + " blocks");
    const std::vector<uint32_t> order = blockOrder(nbx, nby);
    const std::vector<int> shardOf = dealBlocks(nbx, nby, nShards, c->blockWeights);
    std::vector<uint32_t> blockOf;
    std::vector<int32_t> localOf(order.size(), -1);
    for (size_t i = 0; i < order.size(); ++i) /* a shard's blocks in Hilbert order (locality) */
        if (shardOf[order[i]] == shard) {
            localOf[order[i]] = (int32_t) blockOf.size();
            blockOf.push_back(order[i]);
        }
    const int n = (int) order.size();
    if (n > c->ownCap) {
        if (c->dBlockOf) (void) hipFree(c->dBlockOf);
        if (c->dLocalOf) (void) hipFree(c->dLocalOf);
        if (c->dBlockCost) (void) hipFree(c->dBlockCost);
        c->dBlockOf = nullptr;
        c->dLocalOf = nullptr;
        c->dBlockCost = nullptr;
        c->ownCap = 0;
        HIPCHK(c, hipMalloc((void **) &c->dBlockOf, n * sizeof(uint32_t)));
        HIPCHK(c, hipMalloc((void **) &c->dLocalOf, n * sizeof(int32_t)));
        /* HPT_COST_STRIPES stripes of n counters, + a snapshot of them per wave */
        HIPCHK(c, hipMalloc((void **) &c->dBlockCost, 2 * HPT_COST_STRIPES * n * sizeof(uint32_t)));
        c->ownCap = n;
    }
    if (!blockOf.empty())
        HIPCHK(c, hipMemcpy(c->dBlockOf, blockOf.data(), blockOf.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->dLocalOf, localOf.data(), localOf.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(c->dBlockCost, 0, HPT_COST_STRIPES * c->ownCap * sizeof(uint32_t))); /* costs are per ownership */
    c->ownW = W, c->ownH = H, c->ownShard = shard, c->ownShards = nShards, c->ownLocal = (int) blockOf.size();
    c->ownWeights = c->weightsVersion;
    c->ownBlocks.assign(blockOf.begin(), blockOf.end());
    return HPT_OK;
}

/* ---- the wavefront driver ---- */

/* HIP event timing of a render call's launches, per kernel class (hpt_stats::ms_*).  The event
   pairs come from the context's pool, strictly in order */
struct WaveTimer {
    enum Stage { Camera, Primary, Shade, Post, Gather, Tail, TracePacket, Trace, StageCount };
    struct Mark {
        size_t evUsed, pairs[StageCount];
    };
    hpt_context *c = nullptr;
    bool on = false; /* collect_stats != 0 */
    /* collect_stats 3: events around the traversal launches only (k_trace, k_trace_packet): each
       event is a packet between two launches, and a frame of 22 launches pays ~4 us per event */
    bool traceOnly = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[StageCount];
    size_t evUsed = 0;

    template <typename F> hipError_t timed(Stage st, F fn) {
        if (!on || (traceOnly && st != Trace && st != TracePacket)) return fn();
        hipEvent_t a = takeEvent(c, evUsed), b = takeEvent(c, evUsed);
        (void) hipEventRecord(a, c->stream);
        hipError_t e = fn();
        (void) hipEventRecord(b, c->stream);
        ev[st].push_back({a, b});
        return e;
    }
    Mark mark() const {
        Mark m;
        m.evUsed = evUsed;
        for (int i = 0; i < StageCount; ++i) m.pairs[i] = ev[i].size();
        return m;
    }
    void rollback(const Mark &m) { /* the events since the mark back to the pool */
        evUsed = m.evUsed;
        for (int i = 0; i < StageCount; ++i) ev[i].resize(m.pairs[i]);
    }
    double ms(Stage st) const {
        double tot = 0;
        for (auto &p : ev[st]) {
            float ms = 0;
            (void) hipEventElapsedTime(&ms, p.first, p.second);
            tot += ms;
        }
        return tot;
    }
    void publish(hpt_stats &o) const {
        if (!on) return;
        o.ms_camera = ms(Camera);
        o.ms_primary = ms(Primary);
        o.ms_shade = ms(Shade);
        o.ms_post = ms(Post);
        o.ms_gather = ms(Gather);
        o.ms_tail = ms(Tail);
        o.ms_trace_packet = ms(TracePacket);
        o.packet_launches = ev[TracePacket].size();
        o.ms_trace = ms(Trace);
        o.trace_launches = ev[Trace].size();
    }
};

/* the per-launch reports on stderr */
struct LaunchReporter {
    hpt_context *c = nullptr;
    bool perLaunch = false; /* HPT_TRACE_REPORT=1 with counters on: per-launch traversal counters */
    bool perBounce = false; /* HPT_BOUNCE_REPORT=1 with timing on: per-bounce queue sizes and trace time */
    uint64_t prevSt[HPT_TS_PRIM_SLOTS + 1] = {0, 0, 0, 0, 0, 0, 0, 0}, prevShadow[2] = {0, 0};

    void launch(const char *what) {
        if (!perLaunch) return;
        hipStream_t s = c->stream;
        uint64_t hs[HPT_TS_COUNT];
        if (hipMemcpyAsync(hs, c->dstats, sizeof(hs), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess ||
            hipMemsetAsync(c->dstats + HPT_TS_MAX_ROUNDS, 0, (HPT_TS_RESTARTS + 1 - HPT_TS_MAX_ROUNDS) * 8, s) != hipSuccess)
            return;
        if (c->packets && std::strcmp(what, "camera") == 0) {
            const double rays = (double) std::max<uint64_t>(1, hs[HPT_TS_PACKET_RAYS]);
            std::fprintf(stderr, "[trace] packets  rays %10llu binary nodes/ray %6.2f prims/ray %6.2f exact/ray %5.2f "
                         "util nodes %.3f prims %.3f | fallbacks %llu\n", (unsigned long long) hs[HPT_TS_PACKET_RAYS],
                         hs[HPT_TS_PACKET_NODES] / rays, hs[HPT_TS_PACKET_PRIMS] / rays, hs[HPT_TS_PACKET_EXACT] / rays,
                         hs[HPT_TS_PACKET_NODES] / std::max(1.0, (double) hs[HPT_TS_PACKET_NODE_SLOTS]),
                         hs[HPT_TS_PACKET_PRIMS] / std::max(1.0, (double) hs[HPT_TS_PACKET_PRIM_SLOTS]),
                         (unsigned long long) hs[HPT_TS_PACKET_FALLBACKS]);
            return;
        }
        uint64_t d[HPT_TS_PRIM_SLOTS + 1];
        for (int i = 0; i <= HPT_TS_PRIM_SLOTS; ++i) d[i] = hs[i] - prevSt[i], prevSt[i] = hs[i];
        const uint64_t dsN = hs[HPT_TS_SHADOW_NODES] - prevShadow[0], dsP = hs[HPT_TS_SHADOW_PRIMS] - prevShadow[1];
        prevShadow[0] = hs[HPT_TS_SHADOW_NODES], prevShadow[1] = hs[HPT_TS_SHADOW_PRIMS];
        const uint64_t nC = d[HPT_TS_CLOSEST_RAYS], nS = d[HPT_TS_SHADOW_RAYS];
        std::fprintf(stderr, "[trace] %-8s shadow rays: nodes/ray %6.2f prims/ray %6.2f | closest rays: nodes/ray %6.2f "
                     "prims/ray %6.2f\n", what, dsN / std::max(1.0, (double) nS), dsP / std::max(1.0, (double) nS),
                     (d[HPT_TS_NODES] - dsN) / std::max(1.0, (double) nC),
                     (d[HPT_TS_PRIMS] - dsP) / std::max(1.0, (double) nC));
        const double rays = (double) (nC + nS);
        std::fprintf(stderr, "[trace] %-8s closest %10llu shadow %10llu nodes/ray %6.2f prims/ray %6.2f exact/ray %5.2f "
                     "util nodes %.3f prims %.3f | max rounds %llu max restarts %llu restarted rays %llu restarts %llu\n", what,
                     (unsigned long long) nC, (unsigned long long) nS, d[HPT_TS_NODES] / std::max(1.0, rays),
                     d[HPT_TS_PRIMS] / std::max(1.0, rays), d[HPT_TS_PRIM_EXACT] / std::max(1.0, rays),
                     d[HPT_TS_NODES] / std::max(1.0, (double) d[HPT_TS_NODE_SLOTS]),
                     d[HPT_TS_PRIMS] / std::max(1.0, (double) d[HPT_TS_PRIM_SLOTS]),
                     (unsigned long long) hs[HPT_TS_MAX_ROUNDS], (unsigned long long) hs[HPT_TS_MAX_RESTARTS],
                     (unsigned long long) hs[HPT_TS_RESTARTED_RAYS], (unsigned long long) hs[HPT_TS_RESTARTS]);
    }
    /* after bounce b's trace launch */
    void bounce(const WaveTimer &t, int b, uint64_t grid) {
        if (!perBounce || !t.on || t.ev[WaveTimer::Trace].empty()) return;
        float ms = 0;
        (void) hipStreamSynchronize(c->stream);
        (void) hipEventElapsedTime(&ms, t.ev[WaveTimer::Trace].back().first, t.ev[WaveTimer::Trace].back().second);
        std::fprintf(stderr, "[bounce %d] shade %llu -> trace %.3f ms\n", b, (unsigned long long) grid, ms);
    }
};

/* what the waves of one render call share */
struct Frame {
    hpt_context *c = nullptr;
    float4 *dFilm = nullptr;
    bool counted = false; /* collect_stats 2: + traversal counters (k_trace_counted) */
    WaveTimer timer;
    LaunchReporter report;
    uint64_t bounces = 0;
    int maxB = 0;
    int rc = HPT_OK; /* of a wave that ended in WaveError */

    uint32_t *traversalStats() const { return counted ? (uint32_t *) c->dstats : nullptr; }
};

enum WaveResult { WaveDone, WaveAgain /* render this wave again */, WaveError /* Frame::rc */ };

WaveResult renderFailed(Frame &f, hipError_t e) {
    (void) hipStreamSynchronize(f.c->stream);
    f.rc = setErr(f.c, HPT_EDEVICE, std::string("render failed: ") + hipGetErrorString(e));
    return WaveError;
}

/* the wave's counter block to c->hostCnt */
hipError_t readCounters(hpt_context *c) {
    hipError_t e = hipMemcpyAsync(c->hostCnt, c->counters, HPT_Q_COUNT * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e;
}

/* HPT_C_ERROR: a path ran out of Sobol dimensions */
int sobolExhausted(hpt_context *c) {
    return setErr(c, HPT_EINVAL, "Lookup dimension exceeds the direction number table size! You may have "
                                 "to reduce the 'maxDepth' parameter of your integrator.");
}

HptWave waveAt(const hpt_context *c, int nbx, int shard, int nShards, uint64_t slots, int j0, int nSpp) {
    HptWave w;
    w.sppBegin = (uint32_t) j0;
    w.nSpp = (uint32_t) nSpp;
    w.nPaths = (uint32_t) (slots * w.nSpp);
    w.width = c->sc.cam.width;
    w.height = c->sc.cam.height;
    w.nbx = nbx;
    w.shard = shard;
    w.nShards = nShards;
    w.blockOf = c->dBlockOf;
    w.localOf = c->dLocalOf;
    w.doneIf = nullptr;
    w.doneParity = 0;
    return w;
}

/* A wave rendered again after its schedule overflowed must not count twice: the traversal
   counters and block costs of the discarded attempt are rolled back to their snapshot at the
   wave's start (the timing events to WaveTimer::mark). */
int snapshotWave(const Frame &f) {
    hpt_context *c = f.c;
    const size_t costWords = (size_t) HPT_COST_STRIPES * c->ownCap;
    if (f.counted)
        HIPCHK(c, hipMemcpyAsync(c->dstats + HPT_TS_COUNT, c->dstats, HPT_TS_COUNT * 8, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dBlockCost + costWords, c->dBlockCost, costWords * 4, hipMemcpyDeviceToDevice, c->stream));
    return HPT_OK;
}
int restoreWave(const Frame &f) {
    hpt_context *c = f.c;
    const size_t costWords = (size_t) HPT_COST_STRIPES * c->ownCap;
    if (f.counted)
        HIPCHK(c, hipMemcpyAsync(c->dstats, c->dstats + HPT_TS_COUNT, HPT_TS_COUNT * 8, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->dBlockCost, c->dBlockCost + costWords, costWords * 4, hipMemcpyDeviceToDevice, c->stream));
    return HPT_OK;
}

/* C1: every camera sample of the wave to termination in one launch (k_mesh_paths),
   then the film splat; its time is reported as ms_shade */
WaveResult renderMeshWave(Frame &f, const HptWave &w) {
    hpt_context *c = f.c;
    const HptScene &sc = c->sc;
    hipStream_t s = c->stream;
    hipError_t e = f.timer.timed(WaveTimer::Shade, [&] { return hpt_launch_mesh_paths(sc, c->ms, w, c->P, c->counters, s); });
    if (e) return renderFailed(f, e);
    e = f.timer.timed(WaveTimer::Gather, [&] { return hpt_launch_gather(sc, w, c->P, c->partial, f.dFilm, s); });
    if (e) return renderFailed(f, e);
    e = readCounters(c);
    if (e) return renderFailed(f, e);
    if (c->hostCnt[HPT_C_ERROR]) {
        f.rc = sobolExhausted(c);
        return WaveError;
    }
    uint64_t shaded = 0;
    std::memcpy(&shaded, c->hostCnt + HPT_C_BOUNCES, 8);
    f.bounces += shaded;
    c->stats.paths += w.nPaths;
    return WaveDone;
}

/* the bounce control of one hair wave */
struct HairWave {
    const HptWave &w;
    std::array<int64_t, 4> key;  /* the wave in c->schedules */
    const BounceSchedule *known; /* its schedule there (until the key is erased), or none */
    bool ahead;                  /* the bounces of that schedule are launched ahead */
    bool learn;                  /* the wave's schedule is recorded */
    bool fits = true;            /* the schedule launched ahead was the whole wave */
    bool gatheredAhead = false, doneAtFirstRead = false, extended = false;
    BounceSchedule seen;
    int b = 1;                   /* the next bounce */
};

/* the camera pass is bounce 0 (parity 0) */
hipError_t cameraPass(Frame &f, const HptWave &w) {
    hpt_context *c = f.c;
    const HptScene &sc = c->sc;
    hipStream_t s = c->stream;
    uint32_t *C = c->counters, *dst = f.traversalStats();
    uint32_t *curPacket = C + HPT_CURSOR_SET(2), *curOverflow = C + HPT_CURSOR_SET(3);
    hipError_t e = f.timer.timed(WaveTimer::Camera, [&] {
        return hpt_launch_camera(sc, w, c->P, c->qTrace, C + HPT_C_TRACE(0), s);
    });
    if (e) return e;
    /* the camera pass has no shadow rays: qShadow / C[SHADOW(0)] take the rays of overflowing packets */
    e = c->packets ? f.timer.timed(WaveTimer::TracePacket, [&] {
        return hpt_launch_trace_packet(sc, c->P, c->qTrace, C + HPT_C_TRACE(0), curPacket, dst, w.nPaths, c->qShadow,
                                       C + HPT_C_SHADOW(0), s);
    })
                   : f.timer.timed(WaveTimer::Trace, [&] {
                         return hpt_launch_trace_camera(sc, c->P, c->qTrace, C + HPT_C_TRACE(0), curPacket, dst, w.nPaths, s);
                     });
    if (e) return e;
    f.report.launch("camera");
    if (c->packets) {
        /* overflowing packets' rays (none at the shipped configs), their own cursor set */
        e = hpt_launch_trace_overflow(sc, c->P, c->qTrace, c->qShadow, C + HPT_C_SHADOW(0), curOverflow,
                                      std::min<uint64_t>(w.nPaths, 1u << 16), s);
        if (e) return e;
    }
    return f.timer.timed(WaveTimer::Primary, [&] {
        return hpt_launch_primary(sc, c->P, c->qTrace, C + HPT_C_TRACE(0), c->qShade[1], C + HPT_C_SHADE(1), w.nPaths, s);
    });
}

/* bounce hw.b (parity p): shade -> trace -> clear -> post.
   grid: the shade launch's (the trace launch's work is at most twice it, the post's at most it) */
hipError_t wavefrontBounce(Frame &f, const HairWave &hw, uint32_t p, uint64_t grid, uint32_t tailFrom) {
    hpt_context *c = f.c;
    const HptScene &sc = c->sc;
    hipStream_t s = c->stream;
    uint32_t *C = c->counters, *dst = f.traversalStats();
    const uint32_t q = p ^ 1u;
    hipError_t e1 = f.timer.timed(WaveTimer::Shade, [&] {
        return hpt_launch_shade(sc, c->P, c->qShade[p], C + HPT_C_SHADE(p), c->qTrace, C + HPT_C_TRACE(p),
                                c->qShadow, C + HPT_C_SHADOW(p), C, grid, tailFrom, s);
    });
    if (e1) return e1;
    e1 = f.timer.timed(WaveTimer::Trace, [&] {
        return hpt_launch_trace(sc, c->P, c->qTrace, c->qShadow, C + HPT_C_TRACE(p), C + HPT_C_SHADOW(p),
                                C + HPT_CURSOR_SET(p), dst, 2ull * grid, s, C, q);
    });
    if (e1) return e1;
    f.report.launch("bounce");
    f.report.bounce(f.timer, hw.b, grid);
    return f.timer.timed(WaveTimer::Post, [&] {
        return hpt_launch_post(sc, c->P, c->qTrace, C + HPT_C_TRACE(p), c->qShade[q], C + HPT_C_SHADE(q), C, grid, s);
    });
}

/* the bounces of the wave's known schedule, and the k_tail launch that ended it, without
   reading a queue length back; then the gather */
hipError_t launchScheduleAhead(Frame &f, HairWave &hw) {
    hpt_context *c = f.c;
    const HptScene &sc = c->sc;
    hipStream_t s = c->stream;
    uint32_t *C = c->counters;
    const BounceSchedule &k = *hw.known;
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < k.shade.size() && e == hipSuccess; ++i, ++hw.b)
        e = wavefrontBounce(f, hw, (uint32_t) hw.b & 1u, k.shade[i], 0u);
    if (e == hipSuccess && k.tail)
        e = f.timer.timed(WaveTimer::Tail, [&] {
            const uint32_t p = (uint32_t) hw.b & 1u;
            return hpt_launch_tail(sc, c->P, c->qShade[p], C + HPT_C_SHADE(p), C, HPT_ITEMS_ON_DEVICE, c->tailPaths, s);
        });
    if (e) return e;
    /* the gather right behind the schedule, guarded on the device (the wave is done: no
       live path in this bounce's shade queue, or the tail took it; no overflow), so the
       host's counter read-back no longer stands between the last bounce and it */
    if (!f.report.perLaunch) {
        HptWave wg = hw.w;
        wg.doneIf = C;
        wg.doneParity = (uint32_t) hw.b & 1u;
        e = f.timer.timed(WaveTimer::Gather, [&] { return hpt_launch_gather(sc, wg, c->P, c->partial, f.dFilm, s); });
        if (e) return e;
        hw.gatheredAhead = true;
    }
    return hipSuccess;
}

/* from bounce hw.b on, each bounce's queue length read back (grid sizes, the switch to k_tail)
   until no path is live; c->hostCnt holds the wave's final counters */
hipError_t bounceByBounce(Frame &f, HairWave &hw) {
    hpt_context *c = f.c;
    uint32_t *C = c->counters, *hostCnt = c->hostCnt;
    bool firstRead = true;
    for (;; ++hw.b) {
        const uint32_t p = (uint32_t) hw.b & 1u;
        hipError_t e = readCounters(c);
        if (e) return e;
        const uint32_t n = hostCnt[HPT_C_SHADE(p)];
        if (firstRead) hw.doneAtFirstRead = hptWaveDone(hostCnt, p); /* what the early gather's guard saw */
        firstRead = false;
        if (n == 0 || hostCnt[HPT_C_TAIL_PATHS] != 0) return hipSuccess; /* no live path, or k_tail took the rest */
        if (hw.ahead && hw.fits) {
            /* the schedule did not cover the wave (its tail declined, or bounces ran past it):
               re-record it as the part launched ahead plus the bounces read back from here */
            hw.seen.shade = hw.known->shade;
            hw.seen.tail = false;
            hw.known = nullptr;
            c->schedules.erase(hw.key);
            hw.fits = false;
            hw.learn = hw.extended = true;
            c->stats.schedule_extensions++;
        }
        if (n < c->tailPaths) {
            /* few live paths: finish them all in one launch (k_tail) */
            hw.seen.tail = true;
            e = f.timer.timed(WaveTimer::Tail, [&] {
                return hpt_launch_tail(c->sc, c->P, c->qShade[p], C + HPT_C_SHADE(p), C, n, ~0u, c->stream);
            });
            if (e) return e;
            return readCounters(c);
        }
        hw.seen.shade.push_back(n);
        e = wavefrontBounce(f, hw, p, n, 0u);
        if (e) return e;
    }
}

/* what the wave's final counters say about its schedule: the wave is rendered again if a
   bounce launched ahead overflowed, else its schedule is recorded (or re-recorded, extended) */
WaveResult settleSchedule(Frame &f, HairWave &hw) {
    hpt_context *c = f.c;
    if (c->hostCnt[HPT_C_OVERFLOW] && !hw.ahead) {
        (void) hipStreamSynchronize(c->stream);
        f.rc = setErr(c, HPT_EDEVICE, "internal error: a shade grid sized from its read-back queue overflowed");
        return WaveError;
    }
    if (c->hostCnt[HPT_C_OVERFLOW]) {
        /* a bounce launched ahead had more live paths than its schedule's grid: drop the
           schedule and render the wave again, reading every queue length back (the
           film takes a wave's paths only at its gather) */
        c->schedules.erase(hw.key);
        c->stats.waves--;
        c->stats.schedule_misses++;
        return WaveAgain;
    }
    if (hw.learn) {
        /* (the test hooks shorten first recordings only, so an extended schedule is whole) */
        if (c->scheduleTest == 1 && !hw.extended)
            for (auto &n : hw.seen.shade) n = std::max<uint32_t>(1, n / 2);
        if (c->scheduleTest == 2 && !hw.extended && hw.seen.tail && !hw.seen.shade.empty()) hw.seen.shade.pop_back();
        if (c->schedules.size() >= 4096) c->schedules.clear(); /* e.g. a long run of -r passes */
        c->schedules[hw.key] = hw.seen;
    }
    if (hw.ahead && hw.fits) c->stats.waves_ahead++;
    return WaveDone;
}

/* A wave whose schedule is known (the same spp range and shard rendered since the last prepare)
   launches its bounces ahead, each kernel reading its queue length on the device, and the
   k_tail launch that ended it; the device decides whether the tail takes its bounce (the queue
   is shorter than tailPaths) or leaves it to k_shade.  The host reads the counters back once,
   at the end of the schedule, and goes on bounce by bounce from there if paths are still live
   -- a schedule that does not fit costs launches, never paths.  A wave without a schedule reads
   each bounce's queue length back (grid sizes, the switch to k_tail) and records its
   schedule. */
WaveResult renderHairWave(Frame &f, const HptWave &w) {
    hpt_context *c = f.c;
    hipError_t e = cameraPass(f, w);
    if (e) return renderFailed(f, e);
    const std::array<int64_t, 4> key{(int64_t) w.sppBegin, (int64_t) w.nSpp, w.shard, w.nShards};
    const auto known = c->schedules.find(key);
    const bool ahead = c->bounceAhead && !f.report.perLaunch && !f.report.perBounce && known != c->schedules.end();
    HairWave hw{w, key, ahead ? &known->second : nullptr, ahead, c->bounceAhead && !ahead};
    if (ahead) e = launchScheduleAhead(f, hw);
    if (e == hipSuccess) e = bounceByBounce(f, hw);
    if (e) return renderFailed(f, e);
    const WaveResult settled = settleSchedule(f, hw);
    if (settled != WaveDone) return settled;
    /* the wave's bounce statistics, counted on the device */
    uint64_t shaded = 0;
    std::memcpy(&shaded, c->hostCnt + HPT_C_BOUNCES, 8);
    f.bounces += shaded + c->hostCnt[HPT_C_TAIL_BOUNCES]; /* k_tail counts its first bounce too */
    c->stats.tail_paths += c->hostCnt[HPT_C_TAIL_PATHS];
    f.maxB = std::max(f.maxB, (int) c->hostCnt[HPT_C_LAUNCHES]);
    if (c->hostCnt[HPT_C_ERROR]) {
        (void) hipStreamSynchronize(c->stream);
        f.rc = sobolExhausted(c);
        return WaveError;
    }
    if (!(hw.gatheredAhead && hw.doneAtFirstRead)) /* (else the guarded gather launched ahead took the wave) */
        e = f.timer.timed(WaveTimer::Gather, [&] { return hpt_launch_gather(c->sc, w, c->P, c->partial, f.dFilm, c->stream); });
    c->stats.paths += w.nPaths;
    return e ? renderFailed(f, e) : WaveDone;
}

/* the traversal counters of a counted frame to hpt_stats */
int publishTraversalStats(hpt_context *c) {
    uint64_t hs[HPT_TS_COUNT];
    HIPCHK(c, hipMemcpy(hs, c->dstats, sizeof(hs), hipMemcpyDeviceToHost));
    hpt_stats &o = c->stats;
    o.nodes = hs[HPT_TS_NODES];
    o.prims = hs[HPT_TS_PRIMS];
    o.closest_rays = hs[HPT_TS_CLOSEST_RAYS];
    o.shadow_rays = hs[HPT_TS_SHADOW_RAYS];
    o.shadow_unoccluded = hs[HPT_TS_SHADOW_UNOCCLUDED];
    o.prim_exact = hs[HPT_TS_PRIM_EXACT];
    o.node_slots = hs[HPT_TS_NODE_SLOTS];
    o.prim_slots = hs[HPT_TS_PRIM_SLOTS];
    o.max_leaf_rounds = hs[HPT_TS_MAX_ROUNDS];
    o.max_restarts = hs[HPT_TS_MAX_RESTARTS];
    o.restarted_rays = hs[HPT_TS_RESTARTED_RAYS];
    o.packet_nodes = hs[HPT_TS_PACKET_NODES];
    o.packet_prims = hs[HPT_TS_PACKET_PRIMS];
    o.packet_rays = hs[HPT_TS_PACKET_RAYS];
    o.packet_exact = hs[HPT_TS_PACKET_EXACT];
    o.packet_node_slots = hs[HPT_TS_PACKET_NODE_SLOTS];
    o.packet_prim_slots = hs[HPT_TS_PACKET_PRIM_SLOTS];
    o.packet_fallbacks = hs[HPT_TS_PACKET_FALLBACKS];
    o.binary_nodes = hs[HPT_TS_BIN_NODES];
    return HPT_OK;
}

} // namespace

int renderImpl(hpt_context *c, const hpt_render_params *prm, float4 *dFilm) {
    if (c->device == HPT_HOST_ONLY) return setErr(c, HPT_EDEVICE, "host-only context cannot render");
    if (!c->prepared) return setErr(c, HPT_ESTATE, "hpt_prepare() must succeed before rendering");
    auto t0 = std::chrono::steady_clock::now();
    const HptScene &sc = c->sc;
    const int W = sc.cam.width, H = sc.cam.height;
    const int nbx = (W + HPT_BLOCK - 1) / HPT_BLOCK, nby = (H + HPT_BLOCK - 1) / HPT_BLOCK;
    const int nShards = std::max(1, prm->n_shards), shard = prm->shard;
    if (shard < 0 || shard >= nShards) return setErr(c, HPT_EINVAL, "bad shard");
    if (int r0 = ensureOwnership(c, W, H, nbx, nby, shard, nShards)) return r0;
    const int localBlocks = c->ownLocal;
    const uint64_t slots = (uint64_t) localBlocks * 1024u;
    const int sppBegin = prm->spp_begin, sppEnd = prm->spp_end;
    if (sppEnd < sppBegin || sppBegin < 0) return setErr(c, HPT_EINVAL, "bad spp range");
    std::memset(&c->stats, 0, sizeof(c->stats));
    c->samplesSpp = 0;
    if (slots == 0 || sppEnd == sppBegin) return HPT_OK;
    uint32_t nSpp = waveSpp(slots, (uint64_t) (sppEnd - sppBegin), prm->max_wave_paths);
    const uint64_t waveCap = slots * nSpp;
    if (waveCap > 0xffffffffull) return setErr(c, HPT_EINVAL, "wave too large");
    int r = ensureWave(c, waveCap);
    if (r) return r;
    if (int rp = ensurePartial(c, slots)) return rp;
    hipStream_t s = c->stream;
    c->P.blockCost = c->dBlockCost;
    c->P.costStride = (uint32_t) c->ownCap;
    if (!c->scDev) HIPCHK(c, hipMalloc((void **) &c->scDev, sizeof(HptScene)));
    if (c->scShadow.size() != sizeof(HptScene) || std::memcmp(c->scShadow.data(), &c->sc, sizeof(HptScene)) != 0) {
        HIPCHK(c, hipMemcpy(c->scDev, &c->sc, sizeof(HptScene), hipMemcpyHostToDevice));
        c->scShadow.assign((const uint8_t *) &c->sc, (const uint8_t *) &c->sc + sizeof(HptScene));
    }
    Frame f;
    f.c = f.timer.c = f.report.c = c;
    f.dFilm = dFilm;
    f.timer.on = prm->collect_stats != 0; /* HIP event timing per kernel class */
    f.timer.traceOnly = prm->collect_stats == 3;
    f.counted = prm->collect_stats == 2;
    if (f.counted) HIPCHK(c, hipMemsetAsync(c->dstats, 0, HPT_TS_COUNT * 8, s));
    if (int rf = clearFault(c)) return rf;
    f.report.perLaunch = f.counted && std::getenv("HPT_TRACE_REPORT") != nullptr;
    f.report.perBounce = std::getenv("HPT_BOUNCE_REPORT") != nullptr;
    for (int j0 = sppBegin; j0 < sppEnd;) {
        const HptWave w = waveAt(c, nbx, shard, nShards, slots, j0, std::min<int>((int) nSpp, sppEnd - j0));
        c->P.costSpp = w.nSpp;
        c->stats.waves++;
        const WaveTimer::Mark mark = f.timer.mark();
        if (int rs = snapshotWave(f)) return rs;
        HIPCHK(c, hipMemsetAsync(c->counters, 0, HPT_COUNTER_WORDS * 4, s));
        const WaveResult result = c->meshScene ? renderMeshWave(f, w) : renderHairWave(f, w);
        if (result == WaveError) return f.rc;
        if (result == WaveAgain) {
            f.timer.rollback(mark);
            if (int rr = restoreWave(f)) return rr;
            continue;
        }
        j0 += (int) nSpp;
    }
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return setErr(c, HPT_EDEVICE, std::string("render failed: ") + hipGetErrorString(e));
    if (int rf = checkFault(c)) return rf;
    f.timer.publish(c->stats);
    if (f.counted)
        if (int rt = publishTraversalStats(c)) return rt;
    if (c->stats.waves == 1) c->samplesSpp = (uint32_t) (sppEnd - sppBegin); /* P.pos / P.li hold the frame */
    c->stats.bounces = f.bounces;
    c->stats.max_bounces = f.maxB;
    c->stats.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return HPT_OK;
}

extern "C" {

int hpt_render_device(hpt_context *c, const hpt_render_params *prm, void *dfilm) {
    if (!c || !prm || !dfilm) return HPT_EINVAL;
    if (c->device == HPT_HOST_ONLY) return setErr(c, HPT_EDEVICE, "host-only context cannot render");
    HIPCHK(c, hipSetDevice(c->device));
    return renderImpl(c, prm, (float4 *) dfilm);
}

int hpt_render(hpt_context *c, const hpt_render_params *prm, float *film) {
    if (!c || !prm || !film) return HPT_EINVAL;
    if (c->device == HPT_HOST_ONLY) return setErr(c, HPT_EDEVICE, "host-only context cannot render");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t) c->desc.width * c->desc.height;
    float4 *d = nullptr;
    HIPCHK(c, hipMalloc(&d, n * 16));
    hipError_t e = hipMemcpy(d, film, n * 16, hipMemcpyHostToDevice);
    int r = e == hipSuccess ? renderImpl(c, prm, d) : HPT_EDEVICE;
    if (r == HPT_OK) e = hipMemcpy(film, d, n * 16, hipMemcpyDeviceToHost);
    (void) hipFree(d);
    if (r) return r;
    if (e != hipSuccess) return setErr(c, HPT_EDEVICE, hipGetErrorString(e));
    return HPT_OK;
}

/* the image pixel (y * W + x) of pixel slot `slot` of the current ownership tables, -1 when the
   slot lies outside the frame (the last blocks of a frame that is no multiple of 32) */
static int64_t slotPixel(const hpt_context *c, uint64_t slot, int W, int H, int nbx) {
    const uint32_t b = c->ownBlocks[(size_t) (slot >> 10)], inner = (uint32_t) (slot & 1023u);
    const int px = (int) (b % (uint32_t) nbx) * HPT_BLOCK + (int) (inner & 31u);
    const int py = (int) (b / (uint32_t) nbx) * HPT_BLOCK + (int) (inner >> 5);
    return px < W && py < H ? (int64_t) py * W + px : -1;
}

int hpt_film_splat_batch(hpt_context *c, int n_spp, const float *pos, const float *rgb, int shard, int n_shards,
                         uint64_t max_wave_paths, float *film) {
    if (!c || !pos || !rgb || !film || n_spp <= 0) return setErr(c, HPT_EINVAL, "hpt_film_splat_batch: bad arguments");
    if (c->device == HPT_HOST_ONLY) return setErr(c, HPT_EDEVICE, "host-only context cannot render");
    if (!c->prepared) return setErr(c, HPT_ESTATE, "hpt_prepare() must succeed before hpt_film_splat_batch");
    HIPCHK(c, hipSetDevice(c->device));
    const HptScene &sc = c->sc;
    const int W = sc.cam.width, H = sc.cam.height;
    const int nbx = (W + HPT_BLOCK - 1) / HPT_BLOCK, nby = (H + HPT_BLOCK - 1) / HPT_BLOCK;
    const int nShards = std::max(1, n_shards);
    if (shard < 0 || shard >= nShards) return setErr(c, HPT_EINVAL, "bad shard");
    if (int r0 = ensureOwnership(c, W, H, nbx, nby, shard, nShards)) return r0;
    c->samplesSpp = 0; /* the wave buffers are about to hold the caller's samples */
    const uint64_t slots = (uint64_t) c->ownLocal * 1024u;
    if (slots == 0) return HPT_OK;
    /* the waves of an hpt_render of n_spp samples per pixel */
    const uint32_t nSpp = waveSpp(slots, (uint64_t) n_spp, max_wave_paths);
    const uint64_t waveCap = slots * nSpp;
    if (waveCap > 0xffffffffull) return setErr(c, HPT_EINVAL, "wave too large");
    if (int r = ensureWave(c, waveCap)) return r;
    if (int r = ensurePartial(c, slots)) return r;
    hipStream_t s = c->stream;
    const size_t pixels = (size_t) W * H;
    float4 *dFilm = nullptr;
    HIPCHK(c, hipMalloc((void **) &dFilm, pixels * 16));
    hipError_t e = hipMemcpy(dFilm, film, pixels * 16, hipMemcpyHostToDevice);
    std::vector<float> hp((size_t) waveCap * 2), hl((size_t) waveCap * 4);
    for (int j0 = 0; j0 < n_spp && e == hipSuccess; j0 += (int) nSpp) {
        const HptWave w = waveAt(c, nbx, shard, nShards, slots, j0, std::min<int>((int) nSpp, n_spp - j0));
        /* pixel-major image order -> the wave's path ids (slot * nSpp + sample) */
        for (uint64_t slot = 0; slot < slots; ++slot) {
            const int64_t pix = slotPixel(c, slot, W, H, nbx);
            for (uint32_t jj = 0; jj < w.nSpp; ++jj) {
                const size_t id = (size_t) (slot * w.nSpp + jj);
                if (pix < 0) { /* k_splat never reads these */
                    hp[2 * id] = hp[2 * id + 1] = 0.0f;
                    hl[4 * id] = -1.0f, hl[4 * id + 1] = hl[4 * id + 2] = hl[4 * id + 3] = 0.0f;
                    continue;
                }
                const size_t src = (size_t) pix * (size_t) n_spp + (size_t) j0 + jj;
                hp[2 * id] = pos[2 * src], hp[2 * id + 1] = pos[2 * src + 1];
                hl[4 * id] = rgb[3 * src], hl[4 * id + 1] = rgb[3 * src + 1], hl[4 * id + 2] = rgb[3 * src + 2];
                hl[4 * id + 3] = 0.0f;
            }
        }
        e = hipMemcpyAsync(c->P.pos, hp.data(), (size_t) w.nPaths * 8, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(c->P.li, hl.data(), (size_t) w.nPaths * 16, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hpt_launch_gather(sc, w, c->P, c->partial, dFilm, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s); /* hp / hl are filled again for the next wave */
    }
    if (e == hipSuccess) e = hipMemcpy(film, dFilm, pixels * 16, hipMemcpyDeviceToHost);
    (void) hipFree(dFilm);
    if (e != hipSuccess) return setErr(c, HPT_EDEVICE, std::string("hpt_film_splat_batch: ") + hipGetErrorString(e));
    return HPT_OK;
}

int hpt_get_render_samples(hpt_context *c, float *pos, float *rgb, uint64_t *n) {
    if (!c) return HPT_EINVAL;
    if (c->device == HPT_HOST_ONLY) return setErr(c, HPT_EDEVICE, "host-only context cannot render");
    if (!c->prepared || c->samplesSpp == 0)
        return setErr(c, HPT_ESTATE, "hpt_get_render_samples: the last hpt_render was not a single wave of paths "
                                     "(or nothing was rendered since hpt_prepare / hpt_film_splat_batch)");
    const int W = c->sc.cam.width, H = c->sc.cam.height, nbx = (W + HPT_BLOCK - 1) / HPT_BLOCK;
    const uint32_t spp = c->samplesSpp;
    if (n) *n = (uint64_t) W * H * spp;
    if (!pos && !rgb) return HPT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t slots = (uint64_t) c->ownLocal * 1024u, paths = slots * spp;
    std::vector<float> hp((size_t) paths * 2), hl((size_t) paths * 4);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(hp.data(), c->P.pos, (size_t) paths * 8, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(hl.data(), c->P.li, (size_t) paths * 16, hipMemcpyDeviceToHost));
    for (uint64_t slot = 0; slot < slots; ++slot) {
        const int64_t pix = slotPixel(c, slot, W, H, nbx);
        if (pix < 0) continue;
        for (uint32_t jj = 0; jj < spp; ++jj) {
            const size_t id = (size_t) (slot * spp + jj), dst = (size_t) pix * spp + jj;
            if (pos) pos[2 * dst] = hp[2 * id], pos[2 * dst + 1] = hp[2 * id + 1];
            if (rgb) rgb[3 * dst] = hl[4 * id], rgb[3 * dst + 1] = hl[4 * id + 1], rgb[3 * dst + 2] = hl[4 * id + 2];
        }
    }
    return HPT_OK;
}

int hpt_block_deal(int width, int height, int n_shards, const double *weights, int32_t *shard_of_block) {
    if (width <= 0 || height <= 0 || n_shards <= 0 || !shard_of_block) return HPT_EINVAL;
    const int nbx = (width + HPT_BLOCK - 1) / HPT_BLOCK, nby = (height + HPT_BLOCK - 1) / HPT_BLOCK;
    std::vector<double> w;
    if (weights) w.assign(weights, weights + (size_t) nbx * nby);
    /* the deal's sort needs a strict weak order: no NaN (and, as hpt_set_block_weights, no negative
       or infinite weight) */
    for (double x : w)
        if (!(x >= 0.0) || !std::isfinite(x)) return HPT_EINVAL;
    const std::vector<int> s = dealBlocks(nbx, nby, n_shards, w);
    for (size_t i = 0; i < s.size(); ++i) shard_of_block[i] = s[i];
    return HPT_OK;
}

int hpt_set_block_weights(hpt_context *c, const double *weights, int n_blocks) {
    if (!c || n_blocks < 0 || (n_blocks > 0 && !weights)) return HPT_EINVAL;
    for (int i = 0; i < n_blocks; ++i)
        if (!(weights[i] >= 0.0) || !std::isfinite(weights[i]))
            return setErr(c, HPT_EINVAL, "block weights must be finite and >= 0");
    c->blockWeights.assign(weights, weights + n_blocks);
    c->weightsVersion++;
    c->schedules.clear(); /* a shard's waves change with the deal: their bounce schedules do too */
    return HPT_OK;
}

int hpt_get_block_costs(hpt_context *c, uint64_t *costs, int n_blocks) {
    if (!c || !costs || n_blocks < 0) return HPT_EINVAL;
    std::memset(costs, 0, (size_t) n_blocks * sizeof(uint64_t));
    if (c->device == HPT_HOST_ONLY || !c->dBlockCost || c->ownBlocks.empty()) return HPT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t words = (size_t) HPT_COST_STRIPES * c->ownCap;
    std::vector<uint32_t> local(words);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(local.data(), c->dBlockCost, words * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemset(c->dBlockCost, 0, words * 4));
    for (size_t k = 0; k < c->ownBlocks.size(); ++k) {
        uint64_t sum = 0; /* the stripes of block k */
        for (int st = 0; st < HPT_COST_STRIPES; ++st) sum += local[(size_t) st * c->ownCap + k];
        if ((int) c->ownBlocks[k] < n_blocks) costs[c->ownBlocks[k]] = sum;
    }
    return HPT_OK;
}

int hpt_get_stats(hpt_context *c, hpt_stats *o) {
    if (!c || !o) return HPT_EINVAL;
    *o = c->stats;
    return HPT_OK;
}

} /* extern "C" */
