// fer_mp4.hip -- the coded pictures as fragmented MP4 media segments on the device (ferhip_mp4_open, ferhip_mp4_append,
// ferhip_mp4_close, ferhip_mp4_fetch, ferhip_mp4_blocks, ferhip_write_mp4_init; the definition stands in include/ferhip.h).
// Unlike the other framings this one holds many pictures: every stream owns a region of the caller's buffer, and a segment
// grows in it append by append.  What the next append needs to know -- how many sample bytes and samples the stream has, and
// whether it faulted -- is one uint4 per stream in device memory (state[]), read and written by kernels only: the host
// enqueues append after append and never learns where a sample went until the segment is closed.
//
// A sample is the length-prefixed entry of fer_nalpack.hip, so the sizes are its kernels':
//   k_nal_count, k_nal_plan   run as they are (fer_launch_nal_count): every 4096-byte chunk's incoming counter and the 03
//                bytes in front of it, and the entry's size.
//   k_mp4_index  one wavefront per 64 streams, a lane per stream: the entry's size and the stream's state give the sample's
//                destination (place[]), the trun entry -- three words, stored in place at 88 + 12 n --, the faults and the
//                new state.  A stream's state has one writer per launch (its lane) and launches are ordered by the HIP
//                stream: no atomics.
//   k_mp4_emit   grid (chunk, stream), the scan and the LDS image of k_nal_emit: it builds the chunk's output span at the
//                destination's byte phase, which is arbitrary here, and stores it with store_span.  Two chunks (or two
//                samples) that share a 16-byte word each store their own bytes of it.
//   k_mp4_close  one wavefront per stream stores the words of the region's front (fer_mp4_front_word, fer_mp4_host.h) around
//                the trun entries, and the stream's index entry; one more wavefront sums the index's last entry from state[].
// No workgroup waits for another one: the phases are separate launches on one stream.
#include "fer_nal.h"
#include "fer_mp4_host.h"
#include <string.h>
#include <algorithm>

#define MP4_NOWHERE (~0ull)

struct FerMp4Job {
    FerNalJob nal;               // index / dst / cap unused; avcc = 1
    uint8_t *dst;                // 16-byte aligned; stream s owns [s * stride, (s + 1) * stride)
    unsigned long long stride;   // a multiple of 16
    uint32_t K, D;
    const ferhip_mp4_hdr *hdr;   // [n] device
    uint4 *state;                // [n] x = sample bytes so far, y = samples, z = fault, w = NAL unit type of the first sample
    unsigned long long *place;   // [n] where this append's sample goes, from dst; MP4_NOWHERE = no sample
    const uint32_t *npay;        // null, or [n]: stream s takes part in the first npay[s] appends only (ferhip_mp4_blocks)
    uint32_t round;              // the append's number, for npay
    ferhip_mp4_seg *index;       // [n + 1] device (close)
};

__device__ __forceinline__ uint32_t mp4_be(uint32_t x) { return __builtin_bswap32(x); }

__global__ __launch_bounds__(64) void k_mp4_index(FerMp4Job j)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= j.nal.n) return;
    const uint2 e = j.nal.ent[s];  // (entry size, type), (0, 0) for a stream without a picture
    unsigned long long at = MP4_NOWHERE;
    if (e.x != 0u && (!j.npay || j.round < j.npay[s])) {
        uint4 st = j.state[s];
        if (st.z == 0u) {
            if (st.y >= j.K)
                st.z = 2u;
            else if ((unsigned long long)j.D + st.x + e.x > j.stride)
                st.z = 1u;
            else {
                const unsigned long long region = (unsigned long long)s * j.stride;
                at = region + j.D + st.x;
                // st.y < K: the entry ends at 88 + 12 K <= D - 16, inside the region; region and 88 + 12 n are multiples of 4
                uint32_t *t = (uint32_t *)(j.dst + region + 88u + 12u * st.y);
                t[0] = mp4_be(j.hdr[s].duration);
                t[1] = mp4_be(e.x);
                t[2] = mp4_be(fer_mp4_sample_flags(e.y == (uint32_t)FERHIP_NAL_IDR));
                if (st.y == 0u) st.w = e.y;
                st.x += e.x;  // <= stride - D < 2^31
                st.y += 1u;
            }
            j.state[s] = st;
        }
    }
    j.place[s] = at;
}

// LDS image of one chunk's output, as in fer_nalpack.hip: up to 15 bytes of misalignment, the parameter sets, five prefix
// bytes, the chunk and one 03 for every two of its bytes (+ 1 when the incoming counter is 2), rounded up to 16
#define MP4_IMG ((15 + FER_NAL_PS_ROW + 5 + NAL_CHUNK + NAL_CHUNK / 2 + 1 + 15) & ~15)

__global__ __launch_bounds__(NAL_THREADS) void k_mp4_emit(FerMp4Job j)
{
    const int s = blockIdx.y;
    const unsigned long long at = j.place[s];
    if (at == MP4_NOWHERE) return;  // no picture, or a faulted stream: k_mp4_index has checked that [at, at + bytes) lies in the region
    const uint2 ent = j.nal.ent[s];
    const uint32_t bytes = ent.x, type = ent.y;
    const uint32_t len = nal_len(j.nal, s);
    const uint32_t nch = max((len + NAL_CHUNK - 1) / NAL_CHUNK, 1u);  // an empty payload still has its five prefix bytes
    const uint32_t pslen = (j.nal.ps && type == (uint32_t)FERHIP_NAL_IDR) ? j.nal.ps[(size_t)s * FER_NAL_PS_ROW + FER_NAL_PS_ROW - 1] : 0u;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __shared__ uint4 wtot[NAL_THREADS / 64];
    __shared__ __attribute__((aligned(16))) uint8_t img[MP4_IMG];
    for (uint32_t chunk = blockIdx.x; chunk < nch; chunk += gridDim.x) {
        int nvalid;
        const uint4 v = nal_load(j.nal, s, len, chunk, tid, nvalid);
        const uint4 incl = wave_scan(nal_piece(v, nvalid), lane, NalCompose());
        wg_put(wtot, incl, wave, lane);
        uint4 excl = wave_excl(incl, lane, nal_identity());
        // chunk 0 starts from counter 0 with nothing inserted in front of it
        const uint2 cin = chunk ? j.nal.cin[(size_t)s * j.nal.nchmax + chunk] : make_uint2(0u, 0u);
        __syncthreads();
        const uint4 pre = wg_front(wtot, wave, nal_identity(), NalCompose());
        const uint4 tot = wg_total(wtot, NalCompose());
        excl = NalCompose()(pre, excl);
        // the chunk's span of the output: [a, a + n), staged in img at [sh, sh + n) so that 16-byte words line up
        const uint32_t head = chunk ? 0u : pslen + 5u;
        const unsigned long long a = at + (chunk ? (unsigned long long)pslen + 5ull + (unsigned long long)chunk * NAL_CHUNK + cin.y : 0ull);
        const uint32_t sh = (uint32_t)a & 15u;
        const uint32_t nin = len > chunk * NAL_CHUNK ? min((uint32_t)NAL_CHUNK, len - chunk * NAL_CHUNK) : 0u;
        const uint32_t n = head + nin + nal_cnt(tot, cin.x);
        if (!chunk) {
            if ((uint32_t)tid < pslen) {
                const uint8_t *row = j.nal.ps + (size_t)s * FER_NAL_PS_ROW;
                uint8_t b = row[tid];
                // the row's two start codes become the lengths of the SPS and the PPS unit
                const uint32_t pps = row[FER_NAL_PS_ROW - 2];
                if ((uint32_t)tid < 4u) b = (uint8_t)((pps - 4u) >> (8u * (3u - (uint32_t)tid)));
                if ((uint32_t)tid >= pps && (uint32_t)tid < pps + 4u) b = (uint8_t)((pslen - pps - 4u) >> (8u * (3u - ((uint32_t)tid - pps))));
                img[sh + tid] = b;
            }
            if ((uint32_t)tid >= pslen && (uint32_t)tid < pslen + 5u) {
                const uint32_t k = (uint32_t)tid - pslen;
                const uint32_t ulen = bytes - pslen - 4u;  // header byte + escaped payload
                img[sh + tid] = k < 4u ? (uint8_t)(ulen >> (8u * (3u - k))) : (uint8_t)(1u << 5 | (type & 31u));
            }
        }
        {
            uint32_t z = nal_out(excl, cin.x);
            uint32_t p = sh + head + (uint32_t)tid * 16u + nal_cnt(excl, cin.x);
#define NAL_DWORD(w, k)                                    \
    _Pragma("unroll") for (int q = 0; q < 4; q++)          \
    {                                                      \
        if (4 * (k) + q < nvalid) {                        \
            const uint32_t b = ((w) >> (8 * q)) & 0xffu;   \
            if (nal_step(b, z)) img[p++] = 3;              \
            img[p++] = (uint8_t)b;                         \
        }                                                  \
    }
            NAL_DWORD(v.x, 0)
            NAL_DWORD(v.y, 1)
            NAL_DWORD(v.z, 2)
            NAL_DWORD(v.w, 3)
#undef NAL_DWORD
        }
        __syncthreads();
        // a + n <= at + bytes <= the region's end (k_mp4_index): nothing to cut; dst and a - sh are multiples of 16
        store_span<NAL_THREADS>(j.dst + (a - sh), img, sh, sh + n);
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_mp4_close(FerMp4Job j)
{
    const int s = blockIdx.x, lane = threadIdx.x, S = j.nal.n;
    if (s == S) {  // the last entry: sums over state[], which no workgroup of this launch writes
        uint32_t streams = 0u, samples = 0u, fault = 0u;
        for (int t = lane; t < S; t += 64) {
            const uint4 st = j.state[t];
            streams += st.y ? 1u : 0u;
            samples += st.y;
            fault |= st.z;
        }
        streams = __shfl(wave_scan(streams, lane, ScanAdd()), 63);
        samples = __shfl(wave_scan(samples, lane, ScanAdd()), 63);
        const uint32_t f = (__ballot(fault & 1u) ? 1u : 0u) | (__ballot(fault & 2u) ? 2u : 0u);
        if (lane == 0) {
            ferhip_mp4_seg g;
            g.offset = 0ull, g.bytes = streams, g.nsamples = samples, g.first_nal_type = 0, g.fault = f;
            j.index[S] = g;
        }
        return;
    }
    const uint4 st = j.state[s];
    const unsigned long long region = (unsigned long long)s * j.stride;
    if (lane == 0) {
        ferhip_mp4_seg g;
        g.offset = (st.y || st.z) ? region : 0ull;
        g.bytes = st.y ? j.D + st.x : 0u;
        g.nsamples = st.y;
        g.first_nal_type = st.y ? (int32_t)st.w : 0;
        g.fault = st.z;
        j.index[s] = g;
    }
    if (st.y == 0u) return;  // nothing of the region is written
    const ferhip_mp4_hdr h = j.hdr[s];
    uint32_t *front = (uint32_t *)(j.dst + region);
    for (uint32_t w = (uint32_t)lane; w < j.D / 4u; w += 64u) {  // D <= stride - 16
        bool keep;
        const uint32_t x = fer_mp4_front_word(w, st.y, j.D, st.x, h.decode_time, h.sequence, &keep);
        if (!keep) front[w] = mp4_be(x);
    }
}

// count + plan + index + emit of one append
static void mp4_launch_append(const FerMp4Job &j, hipStream_t st)
{
    fer_launch_nal_count(j.nal, st);
    hipLaunchKernelGGL(k_mp4_index, dim3((unsigned)((j.nal.n + 63) / 64)), dim3(64), 0, st, j);
    hipLaunchKernelGGL(k_mp4_emit, dim3(nal_grid_x(j.nal), j.nal.n), dim3(NAL_THREADS), 0, st, j);
}

static void mp4_launch_close(const FerMp4Job &j, hipStream_t st) { hipLaunchKernelGGL(k_mp4_close, dim3(j.nal.n + 1), dim3(64), 0, st, j); }

static bool mp4_geometry_ok(int max_samples, size_t stride)
{
    if (max_samples < 1 || (unsigned)max_samples > FER_MP4_KMAX || (stride & 15) || stride >= ((size_t)1 << 31)) return false;
    return stride >= (size_t)fer_mp4_data_offset((uint32_t)max_samples) + 16;
}

// ---- host side: an encoder context's segment
static void mp4_job(ferhip_ctx *c, FerMp4Job &j)
{
    j.dst = c->mp4_dst;
    j.stride = c->mp4_stride;
    j.K = (uint32_t)c->mp4_K;
    j.D = fer_mp4_data_offset(j.K);
    j.hdr = c->d_mp4_hdr;
    j.state = c->mp4_state;
    j.place = c->mp4_place;
    j.npay = nullptr;
    j.round = 0u;
    j.index = c->mp4_index;
}

extern "C" int ferhip_mp4_open(ferhip_ctx *c, int flags, int max_samples, const ferhip_mp4_hdr *hdr, void *d_dst, size_t stride)
{
    static_assert(sizeof(ferhip_mp4_hdr) == 16 && sizeof(ferhip_mp4_seg) == 24, "ABI");
    if (!c || !hdr || !d_dst || (flags & ~FERHIP_AU_PARAM_SETS) || ((uintptr_t)d_dst & 15) || !mp4_geometry_ok(max_samples, stride))
        return FERHIP_E_ARG;
    if (c->mp4_open) return FERHIP_E_STATE;
    (void)hipSetDevice(c->device);
    const int S = c->d.S;
    if (!c->mp4_ready) {  // dalloc, halloc and the ring keep what exists: a call after a failed one allocates what is missing
        if (dalloc(c, &c->mp4_state, (size_t)S) || dalloc(c, &c->mp4_place, (size_t)S) || dalloc(c, &c->d_mp4_hdr, (size_t)S) ||
            dalloc(c, &c->mp4_index, (size_t)S + 1) || halloc(c, &c->h_mp4_index, (size_t)S + 1) ||
            hipDeviceSynchronize() != hipSuccess ||  // dalloc clears on the null stream
            c->mp4_ring.create((size_t)S * sizeof(ferhip_mp4_hdr))) {
            (void)hipGetLastError();
            fprintf(stderr, "ferhip: could not allocate the MP4 buffers\n");
            return FERHIP_E_HIP;
        }
        c->mp4_ready = true;
    }
    void *slot = c->mp4_ring.next();
    if (!slot) return FERHIP_E_HIP;
    memcpy(slot, hdr, (size_t)S * sizeof(ferhip_mp4_hdr));
    CK(hipMemcpyAsync(c->d_mp4_hdr, slot, (size_t)S * sizeof(ferhip_mp4_hdr), hipMemcpyHostToDevice, c->st));
    if (int rc = c->mp4_ring.sent(c->st)) return rc;
    CK(hipMemsetAsync(c->mp4_state, 0, (size_t)S * sizeof(uint4), c->st));
    c->mp4_dst = (uint8_t *)d_dst;
    c->mp4_stride = stride;
    c->mp4_K = max_samples;
    c->mp4_flags = flags;
    c->mp4_appended = false;
    c->mp4_open = true;
    return 0;
}

extern "C" int ferhip_mp4_append(ferhip_ctx *c)
{
    if (!c) return FERHIP_E_ARG;
    if (!c->mp4_open || (c->mp4_appended && c->mp4_serial == c->pic_serial)) return FERHIP_E_STATE;
    FerMp4Job j;
    // the sizes' buffers and the parameter set table exist after the segment's first append
    int rc = fer_nal_prepare(c, FERHIP_AU_AVCC | c->mp4_flags, j.nal);
    if (rc) return rc;
    mp4_job(c, j);
    mp4_launch_append(j, c->st);
    CK(hipGetLastError());
    c->mp4_appended = true;
    c->mp4_serial = c->pic_serial;
    return 0;
}

static int mp4_close(ferhip_ctx *c, ferhip_mp4_seg *d_index)
{
    FerMp4Job j{};
    j.nal.n = c->d.S;
    mp4_job(c, j);
    j.index = d_index;
    (void)hipSetDevice(c->device);
    mp4_launch_close(j, c->st);
    c->mp4_open = false;
    CK(hipGetLastError());
    return 0;
}

extern "C" int ferhip_mp4_close(ferhip_ctx *c, ferhip_mp4_seg *d_index)
{
    if (!c || !d_index || ((uintptr_t)d_index & 7)) return FERHIP_E_ARG;
    if (!c->mp4_open) return FERHIP_E_STATE;
    return mp4_close(c, d_index);
}

extern "C" int ferhip_mp4_fetch(ferhip_ctx *c, void *h_dst, size_t cap, ferhip_mp4_seg *h_index)
{
    if (!c || !h_index || (!h_dst && cap)) return FERHIP_E_ARG;
    if (!c->mp4_open) return FERHIP_E_STATE;
    const int S = c->d.S;
    const uint8_t *dst = c->mp4_dst;
    if (int rc = mp4_close(c, c->mp4_index)) return rc;
    CK(hipMemcpyAsync(c->h_mp4_index, c->mp4_index, sizeof(ferhip_mp4_seg) * (S + 1), hipMemcpyDeviceToHost, c->st));
    CK(hipStreamSynchronize(c->st));
    size_t total = 0;
    std::vector<size_t> from(S);
    for (int s = 0; s < S; s++) {
        ferhip_mp4_seg g = c->h_mp4_index[s];
        from[s] = (size_t)g.offset;
        g.offset = (g.bytes || g.fault) ? total : 0;
        total += g.bytes;
        h_index[s] = g;
    }
    h_index[S] = c->h_mp4_index[S];
    if (total > cap) return FERHIP_E_ARG;
    for (int s = 0; s < S; s++)
        if (h_index[s].bytes)
            CK(hipMemcpyAsync((uint8_t *)h_dst + h_index[s].offset, dst + from[s], h_index[s].bytes, hipMemcpyDeviceToHost, c->st));
    CK(hipStreamSynchronize(c->st));
    return 0;
}

extern "C" size_t ferhip_write_mp4_init(ferhip_ctx *c, int s, uint32_t timescale, uint8_t *out, size_t cap)
{
    if (!c || !out || s < 0 || s >= c->d.S || timescale == 0) return 0;
    uint8_t rbsp[64], sps[2 * (5 + 96)], pps[2 * (5 + 96)];
    size_t n = ferhip_write_sps(c, rbsp, sizeof rbsp);
    if (n < 3) return 0;
    const size_t ns = ferhip_write_nal(1, 7, rbsp, n, sps) - 4;  // the unit behind its start code
    n = ferhip_write_pps_stream(c, s, rbsp, sizeof rbsp);
    if (n == 0) return 0;
    const size_t np = ferhip_write_nal(1, 8, rbsp, n, pps) - 4;
    const std::vector<uint8_t> seg = fer_mp4_init_segment(sps + 4, ns, pps + 4, np, c->disp_w, c->disp_h, timescale);
    if (seg.empty() || seg.size() > cap) return 0;
    memcpy(out, seg.data(), seg.size());
    return seg.size();
}

// known-answer surface: host payloads through the same kernels, on the null stream with buffers of its own.  Segment g takes
// payloads g m .. g m + m - 1; append i of the m takes payload g m + i of every segment, so the payloads lie append-major on
// the device: slot i nseg + g.
extern "C" int ferhip_mp4_blocks(const uint8_t *payloads, size_t pstride, const uint32_t *lens, const int32_t *nal_type, size_t n, size_t m,
                                 int max_samples, const ferhip_mp4_hdr *hdr, uint8_t *out, size_t stride, ferhip_mp4_seg *index)
{
    if (!lens || !nal_type || !hdr || !out || !index || n == 0 || n > 65535 || m == 0 || m > 65535 || !mp4_geometry_ok(max_samples, stride))
        return FERHIP_E_ARG;
    uint32_t maxlen = 0;
    for (size_t i = 0; i < n; i++) {
        if (lens[i] > pstride || lens[i] > (1u << 30) || (lens[i] && !payloads)) return FERHIP_E_ARG;
        maxlen = std::max(maxlen, lens[i]);
    }
    const size_t nseg = (n + m - 1) / m, slots = nseg * m;
    const size_t pitch = std::max<size_t>(((size_t)maxlen + 15) & ~(size_t)15, 16);
    const int nchmax = (int)std::max<size_t>(((size_t)maxlen + 4095) / 4096, 1);
    std::vector<uint32_t> hl(slots, 0u), hn(nseg);
    std::vector<int32_t> ht(slots, FERHIP_NAL_SLICE);
    DevBuf<uint8_t> src, dst;
    DevBuf<uint32_t> dl, dn;
    DevBuf<int32_t> dt;
    DevBuf<ferhip_mp4_hdr> dh;
    DevBuf<uint4> summ, state;
    DevBuf<uint2> cin, ent;
    DevBuf<unsigned long long> place;
    DevBuf<ferhip_mp4_seg> idx;
    if (src.reserve(pitch * slots) || dst.reserve(nseg * stride) || dl.reserve(slots) || dn.reserve(nseg) || dt.reserve(slots) || dh.reserve(nseg) ||
        summ.reserve(nseg * nchmax) || state.reserve(nseg) || cin.reserve(nseg * nchmax) || ent.reserve(nseg) || place.reserve(nseg) ||
        idx.reserve(nseg + 1))
        return FERHIP_E_HIP;
    CK(hipMemset(src, 0, pitch * slots));
    for (size_t k = 0; k < n; k++) {
        const size_t g = k / m, i = k % m, slot = i * nseg + g;
        hl[slot] = lens[k];
        ht[slot] = nal_type[k];
        if (lens[k]) CK(hipMemcpy(src + slot * pitch, payloads + k * pstride, lens[k], hipMemcpyHostToDevice));
    }
    for (size_t g = 0; g < nseg; g++) hn[g] = (uint32_t)std::min(m, n - g * m);
    CK(hipMemcpy(dl, hl.data(), sizeof(uint32_t) * slots, hipMemcpyHostToDevice));
    CK(hipMemcpy(dt, ht.data(), sizeof(int32_t) * slots, hipMemcpyHostToDevice));
    CK(hipMemcpy(dn, hn.data(), sizeof(uint32_t) * nseg, hipMemcpyHostToDevice));
    CK(hipMemcpy(dh, hdr, sizeof(ferhip_mp4_hdr) * nseg, hipMemcpyHostToDevice));
    CK(hipMemcpy(dst, out, nseg * stride, hipMemcpyHostToDevice));
    CK(hipMemset(state, 0, sizeof(uint4) * nseg));
    FerMp4Job j;
    j.nal.src_stride = pitch;
    j.nal.hdr = nullptr;
    j.nal.ps = nullptr;
    j.nal.avcc = 1;
    j.nal.n = (int)nseg;
    j.nal.nchmax = nchmax;
    j.nal.summ = summ;
    j.nal.cin = cin;
    j.nal.ent = ent;
    j.nal.index = nullptr;
    j.nal.dst = nullptr;
    j.nal.cap = 0;
    j.dst = dst;
    j.stride = stride;
    j.K = (uint32_t)max_samples;
    j.D = fer_mp4_data_offset(j.K);
    j.hdr = dh;
    j.state = state;
    j.place = place;
    j.npay = dn;
    j.index = idx;
    for (size_t i = 0; i < m; i++) {
        j.nal.src = src + i * nseg * pitch;
        j.nal.lens = dl + i * nseg;
        j.nal.types = dt + i * nseg;
        j.round = (uint32_t)i;
        mp4_launch_append(j, nullptr);
    }
    mp4_launch_close(j, nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, dst, nseg * stride, hipMemcpyDeviceToHost));
    CK(hipMemcpy(index, idx, sizeof(ferhip_mp4_seg) * (nseg + 1), hipMemcpyDeviceToHost));
    return 0;  // the temporaries go with their owners
}

// ---- the way in, host part: the box walk itself is fer_mp4_walk_run (fer_mp4_host.h), driven by split_mp4
extern "C" int ferhip_mp4_find_avcc(const uint8_t *init, size_t n, size_t *off, size_t *len)
{
    if (!init || !off || !len) return FERHIP_E_ARG;
    return fer_mp4_find_avcc(init, n, off, len) ? 0 : FERHIP_E_ARG;
}
