// fer_quality.hip -- SSE and SSIM of every coded picture against its source (ferhip_set_quality): k_quality compares the
// snapshot of the source taken before the picture was reconstructed in place (FerDev::qsrc) with the reconstruction and
// writes one ferhip_quality record per stream into the ring, plus the luma SSE that k_rc_plan reads in QUALITY mode.
// One launch per picture on the context's main stream, after entropy coding (the record carries the RBSP length).
//
// Work of one stream: the luma "tasks" are (window row, 63-block column chunk) pairs, one per wavefront: lane l of the task
// reads the 4x8 column of block column 63 k + l in block rows y and y + 1 (eight dwords of source and eight of
// reconstruction) and reduces each row with v_dot4_u32_u8 to sum a, sum b, sum a^2, sum b^2, sum ab.  The window of lane l
// joins its column with lane l + 1's (one DPP wave shift), so 63 of the 64 lanes own a window.  Luma SSE comes from the
// same sums: sum (a - b)^2 = sum a^2 + sum b^2 - 2 sum ab, over the top block only (plus the bottom one in the last window
// row) and over the columns the chunk owns.  Chroma tasks are 16 bytes of Cb or Cr per lane.  Workgroup g of a stream
// takes the g-th contiguous share of both task lists; workgroups are dealt in XCD bands (xcd_swizzle), so neighbouring
// window rows meet in one L2.
//
// Determinism: every lane adds its tasks in a fixed order, wavefronts reduce by a fixed butterfly, the four wavefronts and
// then the workgroups of a stream are added in index order.  The stream's last workgroup (a ticket) does that final sum.
// No floating-point atomics.
#include "../../include/ferhip.h"
#include "fer_internal.h"

#define Q_WAVES 4
#define DPP_WAVE_SHL1 0x130  // lane i <- lane i+1 over the whole wavefront (lane 63 gets 0)

__device__ __forceinline__ unsigned dot4(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_udot4(a, b, c, false); }

__global__ __launch_bounds__(64 * Q_WAVES) void k_quality(FerDev d, int flags, int slot)
{
    const int s = blockIdx.y;
    if (d.hdr[s * 4 + 3] == FER_PIC_ABSENT) {
        // no picture of this stream in this call (uniform over the workgroup): the row's record says so, q_lsse[s] keeps
        // the SSE of the stream's last picture for k_rc_plan
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            ferhip_quality r;
            r.sse[0] = r.sse[1] = r.sse[2] = 0;
            r.ssim_sum = 0.0;
            r.ssim_windows = 0;
            r.qp = d.qp[s] & 0xff;
            r.nal_type = 0;
            r.rbsp_bytes = 0;
            r.picture = (uint32_t)d.rc[s].npic;  // pictures the stream has coded so far
            d.qring[(size_t)slot * d.S + s] = r;
        }
        return;
    }
    const int G = gridDim.x;
    const int g = (int)xcd_swizzle(blockIdx.x, gridDim.x);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const bool want_ssim = flags & FERHIP_QM_SSIM;
    const int W = d.W, Wb = d.W >> 2, Hb = d.H >> 2;
    const int nch = (Wb - 1 + 62) / 63;  // column chunks with at least one window
    const int L = (Hb - 1) * nch;        // luma tasks
    const uint8_t *srcY = d.qsrc + (size_t)s * d.ysz, *recY = d.curY + (size_t)s * d.ysz;

    unsigned long long sse_y = 0, sse_u = 0, sse_v = 0;
    double ssim = 0.0;

    // ---- luma: wavefront `wave` of workgroup g takes tasks t0 + wave, t0 + wave + Q_WAVES, ... < t1
    {
        const int t0 = (int)((long long)L * g / G), t1 = (int)((long long)L * (g + 1) / G);
        for (int t = t0 + wave; t < t1; t += Q_WAVES) {
            const int wy = t / nch, k = t - wy * nch;
            const int bx = 63 * k + lane;
            const bool col_ok = bx < Wb;
            const int bxc = col_ok ? bx : Wb - 1;  // lanes past the right edge load a valid column and are masked
            const size_t off = (size_t)(4 * wy) * W + 4 * bxc;
            unsigned a[8], b[8];
#pragma unroll
            for (int r = 0; r < 8; r++) {
                a[r] = *(const uint32_t *)(srcY + off + (size_t)r * W);
                b[r] = *(const uint32_t *)(recY + off + (size_t)r * W);
            }
            unsigned sa_t = 0, sb_t = 0, sq_t = 0, sab_t = 0, sa_b = 0, sb_b = 0, sq_b = 0, sab_b = 0;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                sa_t = dot4(a[r], 0x01010101u, sa_t);
                sb_t = dot4(b[r], 0x01010101u, sb_t);
                sq_t = dot4(b[r], b[r], dot4(a[r], a[r], sq_t));
                sab_t = dot4(a[r], b[r], sab_t);
                sa_b = dot4(a[r + 4], 0x01010101u, sa_b);
                sb_b = dot4(b[r + 4], 0x01010101u, sb_b);
                sq_b = dot4(b[r + 4], b[r + 4], dot4(a[r + 4], a[r + 4], sq_b));
                sab_b = dot4(a[r + 4], b[r + 4], sab_b);
            }
            // SSE: each block once -- the column belongs to this chunk unless the next chunk starts there, the bottom
            // block row only in the last window row
            const bool own = col_ok && (lane < 63 || k == nch - 1);
            const unsigned e = (sq_t - 2u * sab_t) + (wy == Hb - 2 ? sq_b - 2u * sab_b : 0u);
            sse_y += own ? e : 0u;
            if (want_ssim) {
                const int s1c = (int)(sa_t + sa_b), s2c = (int)(sb_t + sb_b), ssc = (int)(sq_t + sq_b), s12c = (int)(sab_t + sab_b);
                const int s1 = s1c + FER_DPP(s1c, DPP_WAVE_SHL1), s2 = s2c + FER_DPP(s2c, DPP_WAVE_SHL1);
                const int ss = ssc + FER_DPP(ssc, DPP_WAVE_SHL1), s12 = s12c + FER_DPP(s12c, DPP_WAVE_SHL1);
                const long long S1 = s1, S2 = s2;
                const long long vars = 64ll * ss - S1 * S1 - S2 * S2, covar = 64ll * s12 - S1 * S2;
                const long long num = (2 * S1 * S2 + 416) * (2 * covar + 235963);
                const long long den = (S1 * S1 + S2 * S2 + 416) * (vars + 235963);
                const double v = (double)num / (double)den;
                ssim += (lane < 63 && bx + 1 < Wb) ? v : 0.0;
            }
        }
    }
    // ---- chroma: 16 bytes of Cb (index < n4) or Cr per lane, over the g-th share of the stream's 2 * n4 pieces
    {
        const int n4 = (int)(d.csz >> 4), NC = 2 * n4;
        const int c0 = (int)((long long)NC * g / G), c1 = (int)((long long)NC * (g + 1) / G);
        const size_t cs = (size_t)s * d.csz, pl = (size_t)d.S * d.csz;
        const uint8_t *srcC = d.qsrc + (size_t)d.S * d.ysz + cs, *recC = d.curCb + cs;
        for (int i0 = c0; i0 < c1; i0 += 64 * Q_WAVES) {
            const int i = i0 + tid;
            const bool ok = i < c1;
            const int ic = ok ? i : c0;
            const bool cr = ic >= n4;
            const size_t o = (cr ? pl : 0) + (size_t)(ic - (cr ? n4 : 0)) * 16;
            const uint4 a = *(const uint4 *)(srcC + o), b = *(const uint4 *)(recC + o);
            unsigned q = dot4(a.x, a.x, 0u), x = dot4(a.x, b.x, 0u);
            q = dot4(b.x, b.x, q);
            q = dot4(b.y, b.y, dot4(a.y, a.y, q));
            q = dot4(b.z, b.z, dot4(a.z, a.z, q));
            q = dot4(b.w, b.w, dot4(a.w, a.w, q));
            x = dot4(a.w, b.w, dot4(a.z, b.z, dot4(a.y, b.y, x)));
            const unsigned e = ok ? q - 2u * x : 0u;
            sse_u += cr ? 0u : e;
            sse_v += cr ? e : 0u;
        }
    }
    // ---- wavefront butterfly, then the four wavefronts in order
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        sse_y += __shfl_xor(sse_y, m);
        sse_u += __shfl_xor(sse_u, m);
        sse_v += __shfl_xor(sse_v, m);
        ssim += __shfl_xor(ssim, m);
    }
    __shared__ FerQPart part[Q_WAVES];
    __shared__ int last;
    if (lane == 0) {
        part[wave].sse[0] = sse_y;
        part[wave].sse[1] = sse_u;
        part[wave].sse[2] = sse_v;
        part[wave].ssim = ssim;
    }
    __syncthreads();
    if (tid == 0) {
        FerQPart p = part[0];
        for (int w = 1; w < Q_WAVES; w++) {
            p.sse[0] += part[w].sse[0];
            p.sse[1] += part[w].sse[1];
            p.sse[2] += part[w].sse[2];
            p.ssim += part[w].ssim;
        }
        d.qpart[(size_t)s * G + g] = p;
        __threadfence();
        last = atomicAdd(&d.qticket[s], 1u) == (unsigned)(G - 1);
    }
    __syncthreads();
    if (!last || tid != 0) return;
    // ---- the stream's last workgroup: the G partials in index order, the ring record
    __threadfence();
    FerQPart t = d.qpart[(size_t)s * G];
    for (int k = 1; k < G; k++) {
        const FerQPart p = d.qpart[(size_t)s * G + k];
        t.sse[0] += p.sse[0];
        t.sse[1] += p.sse[1];
        t.sse[2] += p.sse[2];
        t.ssim += p.ssim;
    }
    d.qticket[s] = 0;
    ferhip_quality r;
    r.sse[0] = t.sse[0];
    r.sse[1] = t.sse[1];
    r.sse[2] = t.sse[2];
    r.ssim_sum = want_ssim ? t.ssim : 0.0;
    r.ssim_windows = want_ssim ? (uint32_t)((Wb - 1) * (Hb - 1)) : 0u;
    r.qp = d.qp[s] & 0xff;
    r.nal_type = d.hdr[s * 4 + 3] == 2 ? FERHIP_NAL_IDR : FERHIP_NAL_SLICE;
    r.rbsp_bytes = d.out_bytes[s];
    r.picture = (uint32_t)(d.rc[s].npic - 1);  // k_rc_plan has counted this picture
    d.qring[(size_t)slot * d.S + s] = r;
    d.q_lsse[s] = t.sse[0];
}

// workgroups per stream: a multiple of 8 (one band per XCD), about 2048 in all
int fer_quality_groups(const FerDev &d)
{
    int per = 256 / d.S;
    per = per < 1 ? 1 : (per > 16 ? 16 : per);
    return 8 * per;
}

void fer_launch_quality(const FerDev &d, int flags, int slot, hipStream_t st)
{
    hipLaunchKernelGGL(k_quality, dim3(d.qgroups, d.S), dim3(64 * Q_WAVES), 0, st, d, flags, slot);
}
