// fer_rate.hip -- per-stream QP of every picture (ferhip_set_rate): k_rc_plan picks each stream's QP on the device from the
// RBSP length (ABR) or the luma SSE (QUALITY, written by k_quality) of its last picture, so that the picture pipeline needs
// no host synchronisation for rate control.  One lane per stream; runs on the context's main stream after the slice headers
// have been uploaded and before the first launch that reads FerDev::qp or FerDev::hdr.
#include "../../include/ferhip.h"
#include "fer_internal.h"

static __constant__ uint8_t c_qpc_tab[52] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17,
                                             18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29, 30, 31, 32, 32, 33,
                                             34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39};
// round(2^16 * 2^(k/6))
static __constant__ unsigned c_p6[6] = {65536, 73562, 82570, 92682, 104032, 116772};

// 2^(dq/6) in 16.16 fixed point, floor semantics for negative dq
__device__ __forceinline__ unsigned long long pow2q16(int dq)
{
    const int e = dq >= 0 ? dq / 6 : -((-dq + 5) / 6);
    const unsigned long long m = c_p6[dq - 6 * e];
    return e >= 0 ? m << e : m >> -e;
}

// bits the stream's last picture of type y would have taken at QP q
__device__ __forceinline__ unsigned long long rc_est(const FerRcState &r, int y, int q)
{
    return ((unsigned long long)r.last_bits[y] * pow2q16(r.last_qp[y] - q)) >> 16;
}

// QUALITY: est(y, q) = (last_sse[y] * pow2q16(2 * (q - last_qp[y]))) >> 16 <= target, with the 128-bit product exact
__device__ __forceinline__ bool rc_sse_fits(const FerRcState &r, int y, int q, long long target)
{
    const unsigned long long a = (unsigned long long)r.last_sse[y], m = pow2q16(2 * (q - r.last_qp[y]));
    const unsigned long long lo = a * m, hi = __umul64hi(a, m);
    return (hi >> 16) == 0 && ((lo >> 16) | (hi << 48)) <= (unsigned long long)target;
}

__device__ __forceinline__ int rc_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(64) void k_rc_plan(FerDev d)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= d.S) return;
    const FerRcPar p = d.rc_par[s];
    FerRcState r = d.rc[s];
    const unsigned ptype = d.hdr[s * 4 + 3];
    const int y = ptype == 2 ? 1 : 0;  // 0 = P, 1 = I
    if (p.mode != FERHIP_RC_CQP && r.gen != p.gen) {  // entering ABR or QUALITY
        r.err = 0;
        r.have[0] = r.have[1] = 0;
        r.pending = 0;
        r.gen = p.gen;
    }
    const int last_qp = d.qp[s] & 0xff;
    if (r.pending == 1) {  // (a) account the last picture: it was coded in ABR
        const long long b = 8ll * d.out_bytes[s];
        const int yp = r.prev_type;
        r.err += b - p.target;
        r.last_bits[yp] = b;
        r.last_qp[yp] = last_qp;
        r.have[yp] = 1;
    } else if (r.pending == 2) {  // ... in QUALITY: its luma SSE, written by k_quality behind it on this stream
        const int yp = r.prev_type;
        r.last_sse[yp] = (long long)d.q_lsse[s];
        r.last_qp[yp] = last_qp;
        r.have[yp] = 1;
    }
    if (ptype == FER_PIC_ABSENT) {
        // the stream has no picture in this call: its last picture is accounted above, once (out_bytes[s] and q_lsse[s]
        // belong to that picture only until the next call), no QP is chosen, qp[s] stays the QP of its last picture and
        // nothing is appended to the header.  Its RBSP of this call has length 0.
        r.pending = 0;
        d.rc[s] = r;
        d.out_bytes[s] = 0;
        return;
    }
    // (b) this picture's QP
    int q = p.qp;
    if (p.mode == FERHIP_RC_ABR) {
        const long long lo = p.target / 8 > 1 ? p.target / 8 : 1, hi = 8 * p.target;
        long long T = p.target - r.err / p.window;  // C division truncates toward zero
        T = T < lo ? lo : (T > hi ? hi : T);
        if (y == 0) {
            if (r.have[0]) {
                q = p.qp_max;
                for (int k = p.qp_min; k <= p.qp_max; k++)
                    if (rc_est(r, 0, k) <= (unsigned long long)T) {
                        q = k;
                        break;
                    }
                q = rc_clamp(q, r.last_qp[0] - p.max_step, r.last_qp[0] + p.max_step);
            } else if (r.have[1]) {
                q = r.last_qp[1] + p.ip_offset;
            }
        } else {
            if (r.have[0])
                q = r.last_qp[0] - p.ip_offset;
            else if (r.have[1])
                q = r.last_qp[1];
        }
        q = rc_clamp(q, p.qp_min, p.qp_max);
    } else if (p.mode == FERHIP_RC_QUALITY) {
        if (r.have[y]) {
            q = p.qp_min;
            for (int k = p.qp_max; k >= p.qp_min; k--)
                if (rc_sse_fits(r, y, k, p.tsse)) {
                    q = k;
                    break;
                }
            q = rc_clamp(q, r.last_qp[y] - p.max_step, r.last_qp[y] + p.max_step);
        } else if (r.have[1 - y]) {
            q = r.last_qp[1 - y] + (y == 0 ? p.ip_offset : -p.ip_offset);
        }
        q = rc_clamp(q, p.qp_min, p.qp_max);
    }
    r.pending = p.mode == FERHIP_RC_ABR ? 1 : (p.mode == FERHIP_RC_QUALITY ? 2 : 0);
    r.prev_type = y;
    r.npic++;
    d.rc[s] = r;
    d.qp[s] = q | (int)c_qpc_tab[q] << 8;
    // (c) slice_qp_delta = QP - pic_init_qp closes the slice header (shd_write, F/headers_and_parameter_sets.cpp:232)
    const int dq = q - p.base - 14;
    const unsigned code = dq <= 0 ? (unsigned)(-dq) * 2u : (unsigned)dq * 2u - 1u;  // se(v) -> ue(code)
    const int len = 2 * (31 - __clz((int)(code + 1))) + 1;
    const unsigned n = d.hdr[s * 4 + 2];
    if (n + len > 64) {
        d.status[s] |= FER_ERR_HDR_OVERFLOW;
        return;
    }
    unsigned long long h = ((unsigned long long)d.hdr[s * 4] << 32) | d.hdr[s * 4 + 1];
    h = (h << len) | (code + 1);  // len - 1 zeros, then code + 1 in (len + 1) / 2 bits
    d.hdr[s * 4] = (uint32_t)(h >> 32);
    d.hdr[s * 4 + 1] = (uint32_t)h;
    d.hdr[s * 4 + 2] = n + len;
}

void fer_launch_rc_plan(const FerDev &d, hipStream_t st)
{
    hipLaunchKernelGGL(k_rc_plan, dim3((d.S + 63) / 64), dim3(64), 0, st, d);
}
