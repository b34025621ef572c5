// kernels_merge.hip -- merging the detections of a surface's tiles on gfx950 (the rule and the step: include/zly.h, "Tiles").
//
// One workgroup per GROUP of a call (the tiles of one surface).  A group's sources are slabs of the call, in ascending slab index; the tile table says
// which, and where each tile lies in its surface.  The step, in five phases with workgroup barriers between them -- ONE path for every size:
//   A. candidates: slot = ordinal * cap + position runs over every record a source could hold; the valid ones (position < clamp(n_kept, 0, cap))
//      are compacted (ballot + popcount per wave, wave totals through LDS); a candidate's slot orders like (source slab, position): the tie-break
//      of the order.  Its sort key goes to LDS:
//          k1 = (class ^ 0x80000000) << 32 | ~ord(confidence + 0.0f),   ord = the usual monotone map of fp32 values to u32
//      -- ascending k1 = class ascending as int32, confidence descending as fp32 value (-0 and +0 tie) -- beside its slot;
//   B. a bitonic sort of (k1, slot) in LDS, padded to a power of two; the order is strict, so any correct sort gives THE order;
//   C. the candidates' records are read again in sorted order and their boxes mapped to surface fractions (single fp32 operations: x * w + x0
//      is a product, a sum and a quotient, never an fma); the mapped box's corners and area go to LDS;
//   D. greedy suppression in blocks of 64 sorted positions, as nms_general's crowded classes (kernels_post.hip) but over the whole list, the class
//      test being part of the pair test: (1) all waves evaluate the block's 64 x 64 "suppresses" matrix, one __ballot per row; (2) wave 0 runs the
//      greedy loop over the row masks, starting from the flags that earlier blocks left; (3) all threads test the candidates behind the block
//      (while their class can still equal one of the block's) against the block's survivors, broadcast from registers.  A candidate's fate is decided by the survivors in
//      front of it, in order: the sequential loop of the specification;
//   E. the survivors are compacted in sorted order and the first min(n_kept, cap) written; records at or beyond that count are not touched.
// FP contraction is OFF for this file: the map, the corners, the intersection and the quotient are the operation sequence include/zly.h writes out,
// and iou_cxcywh's (kernels_post.hip) for ZLY_MERGE_IOU.
#include "zly_internal.h"

#pragma clang fp contract(off)

namespace zly {

#define MRG_MAX_WAVES 16          // 1024 threads

struct MrgBox { float x, y, w, h; };

// A mapped box as the pair test needs it: corners and area depend on one box only, so they are computed once per candidate (identical expressions,
// identical values; FP contraction is off) and the pair part per pair -- as BoxC in kernels_post.hip
struct MrgC { float x0, y0, x1, y1, area; };

// step 2 of the rule: the record of a tile (member mb of the tile table) in surface fractions
__device__ __forceinline__ MrgBox mrg_map(const zly_det* d, const int* mb)
{
    const float fx0 = (float)mb[1], fy0 = (float)mb[2], fw = (float)mb[3], fh = (float)mb[4], fW = (float)mb[5], fH = (float)mb[6];
    MrgBox b;
    b.x = (d->x * fw + fx0) / fW;
    b.y = (d->y * fh + fy0) / fH;
    b.w = d->w * fw / fW;
    b.h = d->h * fh / fH;
    return b;
}

// m of the rule for the pair (a earlier in the order, b later); metric 0 = IoU (calculateIoU as iou_cxcywh), 1 = IoS
__device__ __forceinline__ float mrg_measure(const MrgC& a, const MrgC& b, int metric)
{
    const float lo_x = (a.x0 < b.x0) ? b.x0 : a.x0, hi_x = (b.x1 < a.x1) ? b.x1 : a.x1;
    const float lo_y = (a.y0 < b.y0) ? b.y0 : a.y0, hi_y = (b.y1 < a.y1) ? b.y1 : a.y1;
    const float dx = hi_x - lo_x, dy = hi_y - lo_y;
    const float ox = (0.0f < dx) ? dx : 0.0f;
    const float oy = (0.0f < dy) ? dy : 0.0f;
    const float inter = ox * oy;
    if (!(inter > 0.0f)) return 0.0f;           // disjoint or touching boxes: m = 0 / x = 0, or 0 by the rule's guard -- either way not above a thr >= 0: no divide
    if (metric == 0) {
        const float uni = a.area + b.area - inter;
        return (uni > 0) ? inter / uni : 0.0f;
    }
    const float mn = (a.area < b.area) ? a.area : b.area;
    return (mn > 0) ? inter / mn : 0.0f;
}

__device__ __forceinline__ float mrg_rl_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
// lane l's box, broadcast (l wave-uniform)
__device__ __forceinline__ MrgC mrg_rl(const MrgC& c, int l)
{
    MrgC r;
    r.x0 = mrg_rl_f(c.x0, l); r.y0 = mrg_rl_f(c.y0, l); r.x1 = mrg_rl_f(c.x1, l); r.y1 = mrg_rl_f(c.y1, l); r.area = mrg_rl_f(c.area, l);
    return r;
}

// Exclusive prefix of `pred` over the workgroup's threads in thread order, plus *base; *base advances by the total.  Every thread calls it;
// wave_tot: [MRG_MAX_WAVES] in LDS.  Three barriers.
__device__ __forceinline__ int mrg_block_offset(bool pred, int* wave_tot, int* base)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = (blockDim.x + 63) >> 6;
    const unsigned long long mask = __ballot(pred);
    if (lane == 0) wave_tot[wave] = __popcll(mask);
    __syncthreads();
    int off = *base;
    for (int w = 0; w < wave; ++w) off += wave_tot[w];
    off += __popcll(mask & ((1ull << lane) - 1ull));
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < nw; ++w) t += wave_tot[w];
        *base += t;
    }
    __syncthreads();
    return off;
}

// tab: [0 .. n_groups] = offsets of the groups' members in the member list; then 7 ints per member: source slab, x0, y0, w, h, W, H.
// P: the LDS capacity in candidates, a power of two >= every group's members * cap.
__global__ __launch_bounds__(1024) void merge_kernel(const int* __restrict__ tab, int n_groups, const unsigned char* __restrict__ slabs,
                                                     unsigned char* __restrict__ out, int cap, int P, int metric, float thr, uint32_t tag0)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char mrg_dyn[];
    unsigned long long* k1 = reinterpret_cast<unsigned long long*>(mrg_dyn);                      // [P] sort key
    MrgC* box = reinterpret_cast<MrgC*>(mrg_dyn + (size_t)P * 8);                                 // [P] corners and area of the mapped box of sorted position p
    unsigned* idx = reinterpret_cast<unsigned*>(mrg_dyn + (size_t)P * 28);                        // [P] the candidate's slot: the tie-break, and where its record lies
    unsigned char* dead = mrg_dyn + (size_t)P * 32;                                               // [P] suppressed flag of sorted position p
    __shared__ unsigned long long rows[64];
    __shared__ int wave_tot[MRG_MAX_WAVES];
    __shared__ int sh_base, sh_flags;
    __shared__ unsigned sh_alive[2];

    const int g = blockIdx.x;
    // wave, M and the survivor mask are wave-uniform, and the compiler is told so: the v_readlane broadcasts below take their lane index from them
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), nt = blockDim.x, nw = (nt + 63) >> 6;
    const int m_begin = tab[g], m_end = tab[g + 1];
    const int* members = tab + n_groups + 1;
    const int n_slots = (m_end - m_begin) * cap;                       // <= P (checked by the host)
    const size_t slab_bytes = sizeof(zly_slab_header) + (size_t)cap * sizeof(zly_det);
    zly_slab_header* ohdr = reinterpret_cast<zly_slab_header*>(out + (size_t)g * slab_bytes);
    zly_det* odets = reinterpret_cast<zly_det*>(ohdr + 1);

    if (tid == 0) { sh_base = 0; sh_flags = 0; }
    __syncthreads();

    // A. candidates, compacted in slot order
    for (int s0 = 0; s0 < n_slots; s0 += nt) {
        const int slot = s0 + tid;
        bool valid = false;
        const zly_det* src = nullptr;
        if (slot < n_slots) {
            const int ord = slot / cap, pos = slot - ord * cap;
            const unsigned char* slab = slabs + (size_t)members[(size_t)(m_begin + ord) * 7] * slab_bytes;
            const zly_slab_header* h = reinterpret_cast<const zly_slab_header*>(slab);
            valid = pos < h->n_kept;                                   // pos < cap: this is pos < clamp(n_kept, 0, cap)
            if (pos == 0 && (h->flags & ZLY_SLAB_OVERFLOW)) atomicOr(&sh_flags, 1);
            src = reinterpret_cast<const zly_det*>(slab + sizeof(zly_slab_header)) + pos;
        }
        const int c = mrg_block_offset(valid, wave_tot, &sh_base);
        if (valid) {
            const unsigned cb = __float_as_uint(src->confidence + 0.0f);                           // -0 -> +0: they tie as values
            const unsigned ordc = (cb & 0x80000000u) ? ~cb : (cb | 0x80000000u);
            k1[c] = ((unsigned long long)((unsigned)src->class_id ^ 0x80000000u) << 32) | (unsigned long long)(~ordc);
            idx[c] = (unsigned)slot;
        }
    }
    __syncthreads();
    const int M = __builtin_amdgcn_readfirstlane(sh_base);             // workgroup-uniform
    const int src_flags = sh_flags;

    // B. bitonic sort of (k1, idx) over n2 = the power of two at or above M
    int n2 = 1;
    while (n2 < M) n2 <<= 1;
    for (int i = M + tid; i < n2; i += nt) { k1[i] = ~0ull; idx[i] = ~0u; }                        // padding: behind every candidate
    __syncthreads();
    const int np = n2 >> 1;
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int pp = tid; pp < np; pp += nt) {
                const int t = ((pp & ~(j - 1)) << 1) | (pp & (j - 1)), u = t | j;
                const unsigned long long a1 = k1[t], b1 = k1[u];
                const unsigned a2 = idx[t], b2 = idx[u];
                const bool a_first = a1 < b1 || (a1 == b1 && a2 < b2);
                const bool asc = (t & k) == 0;
                if (asc != a_first && !(a1 == b1 && a2 == b2)) { k1[t] = b1; idx[t] = b2; k1[u] = a1; idx[u] = a2; }
            }
            __syncthreads();
        }

    // C. the sorted candidates' boxes, mapped to surface fractions
    for (int p = tid; p < M; p += nt) {
        const int slot = (int)idx[p];
        const int ord = slot / cap, pos = slot - ord * cap;
        const int* mb = members + (size_t)(m_begin + ord) * 7;
        const zly_det* d = reinterpret_cast<const zly_det*>(slabs + (size_t)mb[0] * slab_bytes + sizeof(zly_slab_header)) + pos;
        const MrgBox b = mrg_map(d, mb);
        MrgC c;
        c.x0 = b.x - b.w / 2; c.y0 = b.y - b.h / 2; c.x1 = b.x + b.w / 2; c.y1 = b.y + b.h / 2;
        c.area = b.w * b.h;
        box[p] = c;
        dead[p] = 0;
    }
    __syncthreads();

    // D. greedy suppression in blocks of 64 sorted positions.  Every wave holds the block in registers (lane l = member l), so that a member's box
    //    reaches the lanes by v_readlane broadcasts: the loops over rows and over survivors read no LDS
    for (int i0 = 0; i0 + 1 < M; i0 += 64) {
        const int nb = min(64, M - i0);
        const int me_p = i0 + lane;
        const bool valid = lane < nb;
        MrgC me; me.x0 = me.y0 = me.x1 = me.y1 = me.area = 0.f;
        unsigned me_cls = 0u;
        if (valid) { me = box[me_p]; me_cls = (unsigned)(k1[me_p] >> 32); }
        // (1) row i of the "suppresses" matrix: bit j = member j lies behind member i, has its class and m > thr
        for (int i = wave; i < nb; i += nw) {                          // wave-uniform row
            const MrgC bi = mrg_rl(me, i);
            const unsigned ci = (unsigned)__builtin_amdgcn_readlane((int)me_cls, i);
            const bool sup = valid && lane > i && me_cls == ci && mrg_measure(bi, me, metric) > thr;
            const unsigned long long row = __ballot(sup);
            if (lane == 0) rows[i] = row;
        }
        __syncthreads();
        // (2) the greedy loop among the members, on the row masks alone; the flags carry what earlier blocks' survivors suppressed
        if (wave == 0) {
            unsigned long long alive = __ballot(valid && dead[valid ? me_p : 0] == 0);
            const unsigned long long myrow = valid ? rows[lane] : 0ull;                            // row i in lane i's registers
            const int rlo = (int)(myrow & 0xffffffffull), rhi = (int)(myrow >> 32);
            for (int i = 0; i < nb - 1; ++i) {
                if (!((alive >> i) & 1ull)) continue;                  // wave-uniform
                alive &= ~(((unsigned long long)(unsigned)__builtin_amdgcn_readlane(rhi, i) << 32) | (unsigned long long)(unsigned)__builtin_amdgcn_readlane(rlo, i));
            }
            if (valid && !((alive >> lane) & 1ull)) dead[me_p] = 1;
            if (lane == 0) { sh_alive[0] = (unsigned)(alive & 0xffffffffull); sh_alive[1] = (unsigned)(alive >> 32); }
        }
        __syncthreads();
        // (3) the candidates behind the block against the block's survivors, up to four per thread in registers.  Classes ascend, so behind the
        //     first candidate of a class above the block's last nothing can match.  This is where a crowded group's time goes: every wave walks all
        //     of the block's survivors, about a hundred vector instructions per pair test with its IEEE divide, on the one compute unit a group has
        const unsigned long long alive = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)sh_alive[1]) << 32) |
                                         (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)sh_alive[0]);
        const unsigned last_cls = (unsigned)__builtin_amdgcn_readlane((int)me_cls, nb - 1);
        for (int jb = i0 + 64; jb < M; jb += 4 * nt) {                 // one round for every launch shape launch_merge chooses
            MrgC mine[4];
            unsigned mcls[4];
            bool act[4], kill[4];
            bool any = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = jb + tid + k * nt;
                act[k] = false; kill[k] = false; mcls[k] = 0u;
                mine[k].x0 = mine[k].y0 = mine[k].x1 = mine[k].y1 = mine[k].area = 0.f;
                if (j < M) {
                    mcls[k] = (unsigned)(k1[j] >> 32);
                    if (mcls[k] <= last_cls && dead[j] == 0) { mine[k] = box[j]; act[k] = true; }
                }
                any = any || act[k];
            }
            if (__ballot(any) == 0ull) continue;                       // wave-uniform: nothing of this wave can be suppressed by this block
            for (unsigned long long m = alive; m; m &= m - 1ull) {
                const int i = __builtin_ctzll(m);                      // wave-uniform
                const MrgC bi = mrg_rl(me, i);
                const unsigned ci = (unsigned)__builtin_amdgcn_readlane((int)me_cls, i);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (act[k] && mcls[k] == ci && mrg_measure(bi, mine[k], metric) > thr) { act[k] = false; kill[k] = true; }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (kill[k]) dead[jb + tid + k * nt] = 1;
        }
        __syncthreads();
    }

    // E. survivors in sorted order; the first min(n_kept, cap) are stored
    if (tid == 0) sh_base = 0;
    __syncthreads();
    for (int p0 = 0; p0 < M; p0 += nt) {
        const int p = p0 + tid;
        const bool keep = p < M && dead[p] == 0;
        const int o = mrg_block_offset(keep, wave_tot, &sh_base);
        if (keep && o < cap) {
            const int slot = (int)idx[p];
            const int ord = slot / cap, pos = slot - ord * cap;
            const int* mb = members + (size_t)(m_begin + ord) * 7;
            const zly_det* d = reinterpret_cast<const zly_det*>(slabs + (size_t)mb[0] * slab_bytes + sizeof(zly_slab_header)) + pos;
            const MrgBox b = mrg_map(d, mb);                           // the same operations on the same operands as in phase C: the same bits
            zly_det r;
            r.x = b.x; r.y = b.y; r.w = b.w; r.h = b.h;
            r.confidence = d->confidence; r.class_id = d->class_id;
            r.track_id = 0; r.pad_ = 0; r.timestamp = 0;
            odets[o] = r;
        }
    }
    if (tid == 0) {
        const int kept = sh_base;
        ohdr->n_kept = kept; ohdr->n_candidates = M;
        ohdr->flags = (kept > cap || src_flags) ? ZLY_SLAB_OVERFLOW : 0u;
        ohdr->frame_tag = tag0 + (uint32_t)g;
    }
}

size_t merge_lds_bytes(int P) { return (size_t)P * 33; }

// dynamic LDS above 64 KiB needs an opt-in per kernel; done at every engine's first merge, outside any stream capture
hipError_t merge_init()
{
    return hipFuncSetAttribute((const void*)merge_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)merge_lds_bytes(ZLY_MERGE_MAX_CANDIDATES));
}

hipError_t launch_merge(const int* tab, int n_groups, int max_slots, const void* slabs, void* out, int cap, int metric, float thr, uint32_t tag0, hipStream_t s)
{
    if (n_groups < 1 || cap < 1 || max_slots < 0 || max_slots > ZLY_MERGE_MAX_CANDIDATES || (metric != 0 && metric != 1)) return hipErrorInvalidValue;
    int P = 64;
    while (P < max_slots) P <<= 1;
    // one wave where one block of 64 holds everything; above 256 slots as many waves as a workgroup may have (measured at 512 candidates in 512
    // slots: 148 us with 256 threads, 126 us with 1024; at about 50 candidates 22 against 21 us)
    const int threads = P <= 64 ? 64 : (P <= 256 ? 256 : 1024);
    hipLaunchKernelGGL(merge_kernel, dim3(n_groups), dim3(threads), merge_lds_bytes(P), s, tab, n_groups, (const unsigned char*)slabs, (unsigned char*)out, cap, P,
                       metric, thr, tag0);
    return hipGetLastError();
}

}  // namespace zly
