// kernels_area.hip -- the area-average resize filter (ZLY_FLAG_AREA, include/zly.h "Area resize") as a pre-pass in front of the front kernels.
//
// area_kernel reads the call's request frames -- any format, tight or through frame views -- and writes one model-sized tight BGR frame per request
// into the engine's scratch buffer (padding of a letterbox engine included).  The front kernel of the call then runs on that buffer as on any batch
// of model-sized BGR frames, where its own resize is the identity.  No front kernel changes, and a plain engine never launches this unit.
//
// The kernel is bandwidth-bound: every source byte of a band is read once, the output is tiny beside it.
//   Grid.    blockIdx.y = frame; blockIdx.x = (band of consecutive model rows) x (chunk of at most ZLY_AREA_THREADS model columns).  The format and
//            the view are uniform per workgroup, so the branches on them cost nothing.
//   Loads.   A workgroup walks the source rows its band overlaps.  Each row -- ZLY_AREA_CHUNK_PX source pixels of it at a time -- is staged into LDS,
//            plane by plane, with one 16-byte load per lane on consecutive 16-byte-aligned addresses.  Only a lane whose 16 bytes would leave the
//            plane (its first bytes in front of the region's first sample, its last ones behind the plane's end) loads byte by byte, inside the plane.
//   Double buffering.  The next unit's loads are issued into registers before the current unit is consumed from LDS; one barrier per unit.
//   Accumulation.  One thread per content column sums its horizontal footprint from LDS (converting the format on the way: yuv_device.h) into three
//            int32 -- the two edge columns weighted, the columns between unweighted and multiplied by D once -- then adds wy * hsum into the 64-bit accumulators of the content row in progress.  A source row shared by two content rows of a
//            band is read once: consecutive content rows' footprints overlap in at most one source row, so the last row's sums are simply kept.
//            Only band seams read a row twice.
//   Division.  Once per output byte: a float estimate of the quotient (at most 256, so the estimate is within one) corrected by one exact 64-bit
//            multiply-subtract.
#include "zly_internal.h"
#include "yuv_device.h"
#include "letterbox_device.h"
#include "area_device.h"

namespace zly {

typedef unsigned int area_u32x4 __attribute__((ext_vector_type(4)));

#define AREA_PLANE_LDS 4096                  // LDS bytes per plane and buffer: 256 lanes x 16 bytes
static_assert(ZLY_AREA_CHUNK_PX % 2 == 0, "a staging chunk starts at an even source column (4:2:0 and 4:2:2 chroma)");
static_assert(ZLY_AREA_CHUNK_PX * 4 + 15 < AREA_PLANE_LDS, "a chunk of the widest format plus its alignment slack fits one lane load per thread");
static_assert(AREA_PLANE_LDS == ZLY_AREA_THREADS * 16, "one 16-byte load per lane and plane");

// where a frame's planes lie: first sample, end (one past the last byte that may be read), row pitch
struct AreaPlanes {
    const uint8_t* p[3];
    const uint8_t* end[3];
    unsigned int pitch[3];
    int np;                                  // planes in use
    int fmt;
    unsigned int bpp0;                       // bytes per pixel in plane 0
};

__device__ __forceinline__ AreaPlanes area_planes(const uint8_t* base, const FrameDesc* desc, int n, int f, const FrameDesc& d, int view)
{
    AreaPlanes a;
    const int fmt = desc_fmt(d.src_off);
    const unsigned int w = (unsigned)d.w, h = (unsigned)d.h;
    a.fmt = fmt;
    a.p[0] = base + desc_off(d.src_off);
    a.p[1] = a.p[2] = a.p[0]; a.end[1] = a.end[2] = a.p[0]; a.pitch[1] = a.pitch[2] = 0;
    const bool yuv = pix_is_yuv(fmt), nv12 = fmt == ZLY_PIX_NV12_BT601 || fmt == ZLY_PIX_NV12_BT709;
    a.bpp0 = yuv ? 1u : pix_is_y422(fmt) ? 2u : pix_bpp(fmt);
    a.np = !yuv ? 1 : nv12 ? 2 : 3;
    const unsigned int crow = nv12 ? w : w >> 1;          // bytes of a chroma row
    if (view) {
        const ViewRec r = reinterpret_cast<const ViewRec*>(desc + n)[f];
        a.pitch[0] = (unsigned)r.pitch0;
        if (yuv) {
            a.p[1] = base + r.off1; a.pitch[1] = (unsigned)r.pitch1;
            a.p[2] = base + r.off2; a.pitch[2] = (unsigned)r.pitch2;
        }
    } else {
        a.pitch[0] = w * a.bpp0;
        if (yuv) {
            a.p[1] = a.p[0] + (size_t)w * h; a.pitch[1] = crow;
            a.p[2] = a.p[1] + (size_t)crow * (h >> 1); a.pitch[2] = crow;
        }
    }
    a.end[0] = a.p[0] + (size_t)(h - 1) * a.pitch[0] + (size_t)w * a.bpp0;
    if (yuv) {
        a.end[1] = a.p[1] + (size_t)((h >> 1) - 1) * a.pitch[1] + crow;
        a.end[2] = a.p[2] + (size_t)((h >> 1) - 1) * a.pitch[2] + crow;
    }
    return a;
}

// the bytes of plane pl that hold source columns [xa, xb) of source row j (xa even): first byte and count
__device__ __forceinline__ const uint8_t* area_row_bytes(const AreaPlanes& a, int pl, int j, int xa, int xb, unsigned int& nbytes)
{
    if (pl == 0) {
        const int xe = a.bpp0 == 2u ? (xb + 1) & ~1 : xb;           // 4:2:2: whole macropixels (w is even)
        nbytes = (unsigned)(xe - xa) * a.bpp0;
        return a.p[0] + (size_t)j * a.pitch[0] + (size_t)xa * a.bpp0;
    }
    if (a.np == 2) {                                                // NV12: U, V pairs
        nbytes = (unsigned)(((xb + 1) & ~1) - xa);
        return a.p[1] + (size_t)(j >> 1) * a.pitch[1] + (size_t)xa;
    }
    nbytes = (unsigned)(((xb + 1) >> 1) - (xa >> 1));               // I420: one byte per two columns
    return a.p[pl] + (size_t)(j >> 1) * a.pitch[pl] + (size_t)(xa >> 1);
}

// lane t's 16 bytes of a row segment that starts at g: the aligned vector load where all of it lies inside [lo, hi), single bytes of the plane otherwise
__device__ __forceinline__ area_u32x4 area_load16(const uint8_t* q, const uint8_t* lo, const uint8_t* hi)
{
    if (q >= lo && q + 16 <= hi) return *reinterpret_cast<const area_u32x4*>(q);
    area_u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned int x = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint8_t* c = q + k * 4 + b;
            if (c >= lo && c < hi) x |= (unsigned int)*c << (8 * b);
        }
        v[k] = x;
    }
    return v;
}

// (acc + T/2) / T for acc <= 255 * T, T < 2^28: exact
__device__ __forceinline__ unsigned int area_round_div(unsigned long long acc, unsigned int T, float inv_t)
{
    const unsigned long long num = acc + (T >> 1);
    unsigned int q = (unsigned int)((float)num * inv_t);            // the quotient is at most 255 and the estimate's relative error below 2^-21: within one
    const long long r = (long long)num - (long long)((unsigned long long)q * T);
    if (r < 0) --q; else if (r >= (long long)T) ++q;
    return q;
}

// The format families of the horizontal sum: what a pixel's three values are and where they lie in the staged row.  Uniform per workgroup, so the
// family is chosen outside the pixel loop.
enum { AREA_PACKED = 0, AREA_PACKED32 = 1, AREA_YUV420 = 2, AREA_YUV422 = 3 };      // PACKED32: 4-byte pixels at 4-byte-aligned LDS offsets, one dword read each

// t0, t1, t2 += the weighted sums over source columns [ia, ib] of a staged row (its unit begins at column xa; [ia, ib] lies inside the unit and inside
// sx, the footprint of the thread's content column).  The values are B, G, R for the YUV families and bytes 0, 1, 2 of the pixel for the packed ones.
// The footprint's first and last column carry an edge weight and are taken first; every column between weighs Dx and is summed unweighted.
template <int FAM>
__device__ __forceinline__ void area_row_sums(const uint8_t* L0, const uint8_t* L1, const uint8_t* L2, int fmt, unsigned int bpp, bool nv12, const AreaSpan& sx, int Dx,
                                              int xa, int ia, int ib, int& t0, int& t1, int& t2)
{
    auto fetch = [&](int i, int& c0, int& c1, int& c2) {
        const int rel = i - xa;
        if constexpr (FAM == AREA_PACKED) {
            const uint8_t* q = L0 + (unsigned)rel * bpp;
            c0 = q[0]; c1 = q[1]; c2 = q[2];
        } else if constexpr (FAM == AREA_PACKED32) {
            const unsigned int v = *reinterpret_cast<const unsigned int*>(L0 + (unsigned)rel * 4u);
            c0 = (int)(v & 0xffu); c1 = (int)((v >> 8) & 0xffu); c2 = (int)((v >> 16) & 0xffu);
        } else {
            unsigned int word;                                      // B | G << 8 | R << 16
            if constexpr (FAM == AREA_YUV420) {
                const unsigned int Y = L0[rel];
                unsigned int uv;
                if (nv12) { const uint8_t* q = L1 + (rel & ~1); uv = (unsigned int)q[0] | ((unsigned int)q[1] << 8); }
                else uv = (unsigned int)L1[rel >> 1] | ((unsigned int)L2[rel >> 1] << 8);
                word = yuv_bgr_word(Y, uv, fmt);
            } else {
                const uint8_t* q = L0 + (rel & ~1) * 2;
                const int yo = (rel & 1) * 2;
                const bool uyvy = pix_is_uyvy(fmt);
                const unsigned int Y = uyvy ? q[1 + yo] : q[yo];
                const unsigned int uv = uyvy ? ((unsigned int)q[0] | ((unsigned int)q[2] << 8)) : ((unsigned int)q[1] | ((unsigned int)q[3] << 8));
                word = yuv_bgr_word(Y, uv, y422_matrix(fmt));
            }
            c0 = (int)(word & 0xffu); c1 = (int)((word >> 8) & 0xffu); c2 = (int)(word >> 16);
        }
    };
    int c0, c1, c2;
    if (ia <= ib && ia == sx.i0) {
        const int w = area_weight(sx, Dx, ia);
        fetch(ia, c0, c1, c2);
        t0 += w * c0; t1 += w * c1; t2 += w * c2;
        ++ia;
    }
    if (ia <= ib && ib == sx.i1) {
        const int w = area_weight(sx, Dx, ib);
        fetch(ib, c0, c1, c2);
        t0 += w * c0; t1 += w * c1; t2 += w * c2;
        --ib;
    }
    int s0 = 0, s1 = 0, s2 = 0;
#pragma unroll 2                                                    // left to itself the compiler unrolls by 8: 159 VGPRs, half the waves per SIMD (72 so)
    for (int i = ia; i <= ib; ++i) {
        fetch(i, c0, c1, c2);
        s0 += c0; s1 += c1; s2 += c2;
    }
    t0 += Dx * s0; t1 += Dx * s1; t2 += Dx * s2;
}

struct AreaArgs {
    const uint8_t* src; const FrameDesc* desc; int n, view;
    uint8_t* out;                            // [n][th][tw][3]
    int tw, th, lb;
    int band;                                // model rows per workgroup
    int ncc, cw;                             // column chunks per band, model columns per chunk (<= ZLY_AREA_THREADS)
};

__global__ __launch_bounds__(ZLY_AREA_THREADS) void area_kernel(AreaArgs A)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][3][AREA_PLANE_LDS];
    const int tid = (int)threadIdx.x, f = (int)blockIdx.y;
    const int band = (int)blockIdx.x / A.ncc, cc = (int)blockIdx.x - band * A.ncc;
    const FrameDesc d = A.desc[f];
    const AreaPlanes P = area_planes(A.src, A.desc, A.n, f, d, A.view);
    const int fmt = P.fmt;
    const int Sx = d.w, Sy = d.h;
    int Dx = A.tw, Dy = A.th, pad_x = 0, pad_y = 0;
    if (A.lb) { const LbGeom g = lb_geometry(Sx, Sy, A.tw, A.th); Dx = g.nw; Dy = g.nh; pad_x = g.pad_x; pad_y = g.pad_y; }

    const int my0 = band * A.band, my1 = min(my0 + A.band, A.th);
    const int mx = cc * A.cw + tid;
    const bool col = tid < A.cw && mx < A.tw;                       // this thread owns a model column
    const int cx = mx - pad_x;
    const bool col_in = col && cx >= 0 && cx < Dx;                  // ... which is a content column
    uint8_t* const out = A.out + (size_t)f * A.th * A.tw * 3;

    // padding (a letterbox engine's): every pixel of the band outside the content
    if (col)
        for (int my = my0; my < my1; ++my) {
            const int y = my - pad_y;
            if (col_in && y >= 0 && y < Dy) continue;
            uint8_t* o = out + ((size_t)my * A.tw + mx) * 3;
            o[0] = 114; o[1] = 114; o[2] = 114;
        }

    // content columns and rows of this workgroup, and the source rectangle they cover
    const int c_first = max(cc * A.cw - pad_x, 0), c_last = min(min(cc * A.cw + A.cw, A.tw) - 1 - pad_x, Dx - 1);
    const int y_first = max(my0 - pad_y, 0), y_last = min(my1 - 1 - pad_y, Dy - 1);
    if (c_first > c_last || y_first > y_last) return;               // uniform
    const int xs0 = area_span(Sx, Dx, c_first).i0 & ~1, xs1 = area_span(Sx, Dx, c_last).i1 + 1;
    const int js0 = area_span(Sy, Dy, y_first).i0, js1 = area_span(Sy, Dy, y_last).i1;
    const int nu = (xs1 - xs0 + ZLY_AREA_CHUNK_PX - 1) / ZLY_AREA_CHUNK_PX;        // staging units per source row
    const int total = (js1 - js0 + 1) * nu;

    const AreaSpan sx = area_span(Sx, Dx, col_in ? cx : c_first);
    const unsigned int T = (unsigned)Sx * (unsigned)Sy;
    const float inv_t = 1.0f / (float)T;

    // the loads of unit u into registers: one 16-byte lane load per plane
    area_u32x4 r[3] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
    auto issue = [&](int u) {
        const int j = js0 + u / nu, xa = xs0 + (u % nu) * ZLY_AREA_CHUNK_PX, xb = min(xa + ZLY_AREA_CHUNK_PX, xs1);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            if (pl >= P.np) continue;
            unsigned int nb;
            const uint8_t* g = area_row_bytes(P, pl, j, xa, xb, nb);
            const unsigned int sh = (unsigned int)((size_t)g & 15u);
            if ((unsigned)tid * 16u < sh + nb) r[pl] = area_load16(g - sh + (size_t)tid * 16u, P.p[pl], P.end[pl]);
        }
    };

    int hs0 = 0, hs1 = 0, hs2 = 0;                                  // the current source row's horizontal sums: B, G, R
    unsigned long long a0 = 0, a1 = 0, a2 = 0;                      // the content row in progress
    int y = y_first;
    AreaSpan sy = area_span(Sy, Dy, y);

    issue(0);
    for (int u = 0; u < total; ++u) {
        const int buf = u & 1;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            if (pl < P.np) *reinterpret_cast<area_u32x4*>(&lds[buf][pl][tid * 16]) = r[pl];
        __syncthreads();
        if (u + 1 < total) issue(u + 1);

        const int k = u % nu, j = js0 + u / nu, xa = xs0 + k * ZLY_AREA_CHUNK_PX, xb = min(xa + ZLY_AREA_CHUNK_PX, xs1);
        if (k == 0) { hs0 = 0; hs1 = 0; hs2 = 0; }
        if (col_in) {
            unsigned int nb, sh[3] = {0u, 0u, 0u};
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                if (pl < P.np) sh[pl] = (unsigned int)((size_t)area_row_bytes(P, pl, j, xa, xb, nb) & 15u);
            const uint8_t* L0 = &lds[buf][0][sh[0]];
            const uint8_t* L1 = &lds[buf][1][sh[1]];
            const uint8_t* L2 = &lds[buf][2][sh[2]];
            const int ia = max(sx.i0, xa), ib = min(sx.i1, xb - 1);
            int p0 = 0, p1 = 0, p2 = 0;
            if (pix_is_yuv(fmt)) area_row_sums<AREA_YUV420>(L0, L1, L2, fmt, P.bpp0, P.np == 2, sx, Dx, xa, ia, ib, p0, p1, p2);
            else if (pix_is_y422(fmt)) area_row_sums<AREA_YUV422>(L0, L1, L2, fmt, P.bpp0, false, sx, Dx, xa, ia, ib, p0, p1, p2);
            else if (P.bpp0 == 4u && (sh[0] & 3u) == 0u) area_row_sums<AREA_PACKED32>(L0, L1, L2, fmt, P.bpp0, false, sx, Dx, xa, ia, ib, p0, p1, p2);
            else area_row_sums<AREA_PACKED>(L0, L1, L2, fmt, P.bpp0, false, sx, Dx, xa, ia, ib, p0, p1, p2);
            const bool swap = pix_is_rgb_order(fmt);                // the R-first layouts: the sums of byte 0 are R's (the exchange is linear: once per row, not per pixel)
            hs0 += swap ? p2 : p0; hs1 += p1; hs2 += swap ? p0 : p2;
        }
        if (k != nu - 1) continue;
        // source row j is complete: it belongs to the content row in progress, and may end it and begin the next ones
        while (true) {
            const unsigned int wy = (unsigned int)area_weight(sy, Dy, j);
            a0 += (unsigned long long)wy * (unsigned int)hs0;
            a1 += (unsigned long long)wy * (unsigned int)hs1;
            a2 += (unsigned long long)wy * (unsigned int)hs2;
            if (j != sy.i1) break;
            if (col_in) {
                uint8_t* o = out + ((size_t)(y + pad_y) * A.tw + mx) * 3;
                o[0] = (uint8_t)area_round_div(a0, T, inv_t);
                o[1] = (uint8_t)area_round_div(a1, T, inv_t);
                o[2] = (uint8_t)area_round_div(a2, T, inv_t);
            }
            a0 = a1 = a2 = 0;
            if (++y > y_last) break;
            sy = area_span(Sy, Dy, y);
            if (sy.i0 != j) break;                                  // the next content row begins with the next source row
        }
    }
}

hipError_t launch_area(const uint8_t* src, const FrameDesc* desc, int n, bool view, uint8_t* out, int tw, int th, bool lb, int num_cus, hipStream_t s)
{
    AreaArgs a;
    a.src = src; a.desc = desc; a.n = n; a.view = view ? 1 : 0; a.out = out; a.tw = tw; a.th = th; a.lb = lb ? 1 : 0;
    a.ncc = (tw + ZLY_AREA_THREADS - 1) / ZLY_AREA_THREADS;
    a.cw = (tw + a.ncc - 1) / a.ncc;
    // fewer rows per band where the large band would leave compute units without a workgroup (small batches)
    const long wgs = (long)n * a.ncc * ((th + ZLY_AREA_BAND_ROWS - 1) / ZLY_AREA_BAND_ROWS);
    a.band = wgs >= 2L * num_cus ? ZLY_AREA_BAND_ROWS : ZLY_AREA_BAND_SMALL;
    const dim3 grid((unsigned)(a.ncc * ((th + a.band - 1) / a.band)), (unsigned)n);
    hipLaunchKernelGGL(area_kernel, grid, dim3(ZLY_AREA_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace zly
