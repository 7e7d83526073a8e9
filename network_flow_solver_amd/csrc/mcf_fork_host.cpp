// mcf_fork_host.cpp -- host restatement of the copy kernel of mcf_fork / mcf_restore, test infrastructure only.
//
// The kernel (mcf_engine.hip: k_fork) calls the MCF_HD functions mcf_fork_* of mcf_core.h; this file calls the very same
// functions from plain loops over workgroups, items and lanes, so the CPU test-suite can check that every byte of every
// segment reaches every destination exactly once and that nothing else is written.  It is NOT a CPU path of the library:
// nothing in the package loads it.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "mcf_core.h"

extern "C" {

int mcf_fork_chunk_bytes_host(void) { return MCF_FORK_CHUNK; }
int mcf_fork_group_host(void) { return MCF_FORK_GROUP; }

// Runs the copy of `nseg` segments of lengths bytes[] to `count` destinations with `grid` workgroups, on counters instead
// of memory: writes[(d * nseg + s) * stride + b] is incremented for every write of byte b of segment s of destination d
// (stride >= the longest segment + 16: a write past the end of a segment is counted there, a write further out in
// *outside).  reads[s * stride + b] counts the loads of the source likewise.  Returns 0, or -1 on bad arguments.
int mcf_fork_cover_host(int32_t nseg, const int64_t* bytes, int64_t count, int32_t grid, int64_t stride, uint8_t* writes,
                        uint32_t* reads, int64_t* outside) {
    if (nseg < 0 || count < 0 || grid < 1 || !outside) return -1;
    std::vector<McfForkSeg> seg((size_t)nseg);
    int64_t chunks = 0;
    for (int32_t s = 0; s < nseg; ++s) {
        if (bytes[s] < 0 || bytes[s] + 16 > stride) return -1;
        seg[(size_t)s].src = nullptr; seg[(size_t)s].bytes = bytes[s]; seg[(size_t)s].chunk0 = chunks; seg[(size_t)s].slot = s; seg[(size_t)s].pad = 0;
        chunks += mcf_fork_chunks(bytes[s]);
    }
    *outside = 0;
    const int64_t items = mcf_fork_items(chunks, count);
    auto touch = [&](int64_t d, int32_t s, int64_t off, int64_t len) {
        for (int64_t b = off; b < off + len; ++b) {
            if (b < 0 || b >= stride) { ++*outside; continue; }
            uint8_t& w = writes[(size_t)((d * nseg + s) * stride + b)];
            if (w < 255) ++w;
        }
    };
    for (int32_t wg = 0; wg < grid; ++wg)
        for (int64_t item = wg; item < items; item += grid) {
            int64_t chunk, d_lo, d_hi;
            mcf_fork_item(item, chunks, count, &chunk, &d_lo, &d_hi);
            const int32_t si = mcf_fork_find(seg.data(), nseg, chunk);
            const McfForkSeg& sg = seg[(size_t)si];
            for (int32_t lane = 0; lane < MCF_FORK_THREADS; ++lane) {
                int64_t vec, tail;
                mcf_fork_lane(sg.bytes, chunk - sg.chunk0, lane, &vec, &tail);
                if (vec >= 0) {
                    if (reads) for (int64_t b = vec; b < vec + 16 && b < stride; ++b) ++reads[(size_t)(sg.slot * stride + b)];
                    for (int64_t d = d_lo; d < d_hi; ++d) touch(d, sg.slot, vec, 16);
                }
                if (tail >= 0) {
                    if (reads && tail < stride) ++reads[(size_t)(sg.slot * stride + tail)];
                    for (int64_t d = d_lo; d < d_hi; ++d) touch(d, sg.slot, tail, 1);
                }
            }
        }
    return 0;
}

}  // extern "C"
