// ptx_stream.h -- the streamed-lanes driver (trace_stream) of the trace kernel (ptx_wave.hip:
// trace_queue): the batch stream, the refill threshold and the finalise-and-take loop.  The walk
// itself is FlatWalk's (ptx_device.h), the end of a query end_query (ptx_wave_common.h).  In a
// header of its own so that another kernel can walk a segment's queries the same way (round 6 built
// a fused spatial-rounds kernel on it: bit-exact, but 7 % slower -- DESIGN §9).
#pragma once
#include "ptx_wave_common.h"

namespace ptx {

// ---------------------------------------------------------------- streamed lanes
// The production walk (FlatWalk, ptx_device.h: flattened instances, LDS tables) with LANE REFILL: a
// lane whose query is over takes the next query of the wave's batch stream at once, instead of
// idling until the wave's slowest query of a fixed 64-query batch ends.  What a lane does for one
// query is what trace_core_flat's batch does -- the same steps on the same state, and end_query at
// its end -- so every result is bit-identical.  Only the interleaving across lanes changes: a
// straggler's node loop now runs beside other lanes' new queries.  Lanes whose query is over are
// finalised (result written, or the Visibility walk continued from the transmissive hit) and given
// new queries once at least PTX_STREAM_REFILL of them wait, or when no lane is still walking (the
// result write and the ray load then serve many lanes at once).  The stream: the workgroup's
// segment `sj` (`sn` queries), its 64-query batches taken by the workgroup's waves, as their lanes
// need them, through the LDS counter `l_next`.
#ifndef PTX_STREAM_REFILL
#define PTX_STREAM_REFILL 32
#endif
#ifndef PTX_TRACE_STREAM
#define PTX_TRACE_STREAM 1
#endif
template <bool PROF, bool OCC>
__device__ __forceinline__ void trace_stream(const Scene &sc, const SubRoot *subs, const Inst *insts, PassEps eps,
                                             uint32_t *stack, CoopLds coop, const WaveBufs &w, float4 *res_all,
                                             uint32_t *l_next, uint32_t sj, uint32_t sn) {
    const uint32_t lane = __lane_id();
    // ---- the batch stream (wave-uniform)
    bool src_done = false;
    uint32_t qbase = 0u, qleft = 0u;  // the current batch's untaken queries: ray slots qbase ..
    // ---- this lane's query and its walk
    bool has = false;
    uint32_t gi = 0u, kind = 0u, seg = 0u;
    float T = 1.0f, remain = 0.0f;
    Ray ray{mk(0.0f, 0.0f, 0.0f), mk(0.0f, 0.0f, 1.0f)};
    Prof pf{};
    FlatWalk wk;
    for (;;) {  // wave-uniform
        // ---- finalise + take new queries, once enough lanes wait or none walks
        const unsigned long long walking = wballot(has && !wk.done);
        const uint32_t waiting = (uint32_t)__popcll(wballot(!(has && !wk.done)));
        if (walking == 0ull || (waiting >= PTX_STREAM_REFILL && !src_done)) {
            if (has && wk.done) {
                if (PROF) wk.count(sc);
                if (end_query(sc, subs, insts, eps, wk.hit(), ray, kind, T, remain, seg, res_all, gi)) has = false;
                else wk.begin(ray, vis_bound(remain));  // the next segment of the same Visibility query
            }
            // new queries for the free lanes, in lane order from the stream
            unsigned long long want = wballot(!has);
            while (want != 0ull && !src_done) {  // wave-uniform
                if (qleft == 0u) {  // the workgroup's next batch of its segment
                    uint32_t b = 0u;
                    if (lane == 0u) b = __hip_atomic_fetch_add(l_next, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
                    if (b * 64u >= sn) {
                        src_done = true;
                        break;
                    }
                    qbase = sj * w.ray_stride + b * 64u;
                    qleft = min(64u, sn - b * 64u);
                }
                const uint32_t m = (uint32_t)__popcll(want), take = min(m, qleft);
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(want >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)want, 0u));
                if (!has && rank < take) {
                    gi = qbase + rank;
                    const float4 a = w.rays[2u * gi], b = w.rays[2u * gi + 1u];
                    ray = Ray{mk(a.x, a.y, a.z), mk(b.x, b.y, b.z)};
                    remain = a.w;
                    kind = asu(b.w);
                    T = 1.0f;
                    seg = 0u;
                    has = true;
                    wk.begin(ray, kind != Q_CLOSEST ? vis_bound(remain) : 1e10f);
                }
                qbase += take;
                qleft -= take;
                want = wballot(!has);
            }
            if (wballot(has) == 0ull) break;  // the stream is drained and every query written
        }
        wk.refill<PROF>(sc, subs, insts, ray, pf);
        wk.nodes<PROF>(sc, subs, stack, WB, pf);
        wk.leaves<PROF, OCC>(sc, coop, eps, remain, pf);
    }
    if (PROF) prof_flush(sc, pf);
}

}  // namespace ptx
