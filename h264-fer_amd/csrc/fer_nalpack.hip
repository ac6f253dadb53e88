// fer_nalpack.hip -- Annex-B framing of the coded pictures on the device (ferhip_pack_nal, ferhip_fetch_nal,
// ferhip_frame_nal_blocks): start code, header byte and emulation prevention of writeNAL (F/nal.cpp:261-299) for many
// payloads at once, written 16-byte aligned into one buffer with an index of (offset, bytes, NAL type).
// FERHIP_AU_AVCC: the four bytes in front of every unit are its length (big-endian) instead of 00 00 00 01, nothing else
// changes; the host-side AVCDecoderConfigurationRecord (ferhip_write_avcc_config) stands at the end of the file.
//
// writeNAL's counter takes the values 0, 1 and 2 only and an insertion resets it, so a run of payload bytes is a function
// on three states: for each incoming counter value, how many 03 bytes it inserts and which value it leaves.  These
// functions compose, and composition is associative: a scan.  In closed form, inside a maximal zero run z_0 .. z_{L-1} that
// starts from counter 0 an 03 goes before z_k exactly when k >= 2 and k is even, and before the non-zero byte b that ends
// it exactly when b <= 3, L >= 2 and L is even; tests/nal_model.py states that form and is pinned to the byte loop.
//
//   k_nal_count  grid (chunk, payload): a lane takes 16 payload bytes (masked past the payload's length) and reduces them
//                to their function; the 256 lanes of a workgroup compose theirs in order (wavefront scan by shuffles, the
//                four wavefronts through LDS); one function per 4096-byte chunk goes to HBM.
//   k_nal_plan   one wavefront per payload composes the chunk functions in order into each chunk's incoming counter and
//                the number of 03 bytes in front of it, and the size of the payload's entry.
//   k_nal_index  one wavefront: the exclusive sum over the payloads of the 16-rounded entry sizes = the index.
//   k_nal_emit   grid (chunk, payload): every lane recomputes its function, the same scan gives its incoming counter and
//                output position, the bytes and the inserted 03s are placed in output order in LDS, and the chunk's
//                output span is stored with 16-byte stores; the ragged bytes at its two ends share a 16-byte word with the
//                neighbouring chunk and are stored byte-wise.  Chunk 0 also places the parameter sets (where asked for),
//                the start code -- or the unit's length, which the index holds since k_nal_plan -- and the header byte.  An entry is written only if its 16-byte slots end within `cap`.
// No workgroup waits for another one: the phases are separate launches on one stream.  The scans (wavefront, workgroup,
// chunks of a payload) and the store of a span from LDS are fer_scan.h's, shared with fer_nalsplit.hip; the job, the
// function (NalCompose) and the load are fer_nal.h's, shared with fer_rtp.hip, which runs k_nal_count and k_nal_plan as they
// are (fer_launch_nal_count); what is local is the byte walk.
// The host side follows the kernels: the context's buffers and parameter set table, and the three entry points.
#include "fer_nal.h"
#include <string.h>
#include <algorithm>

// LDS image of one chunk's output: up to 15 bytes of misalignment, the parameter sets, five prefix bytes, the chunk and
// one 03 for every two of its bytes (+ 1 when the incoming counter is 2), rounded up to 16
#define NAL_IMG ((15 + FER_NAL_PS_ROW + 5 + NAL_CHUNK + NAL_CHUNK / 2 + 1 + 15) & ~15)

__global__ __launch_bounds__(NAL_THREADS) void k_nal_count(FerNalJob j)
{
    const int s = blockIdx.y;
    const uint32_t len = nal_len(j, s);  // 0 for a stream without a picture: its workgroups leave here
    const uint32_t nch = (len + NAL_CHUNK - 1) / NAL_CHUNK;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __shared__ uint4 wtot[NAL_THREADS / 64];
    for (uint32_t chunk = blockIdx.x; chunk < nch; chunk += gridDim.x) {
        int nvalid;
        const uint4 v = nal_load(j, s, len, chunk, tid, nvalid);
        wg_put(wtot, wave_scan(nal_piece(v, nvalid), lane, NalCompose()), wave, lane);
        __syncthreads();
        if (tid == 0) j.summ[(size_t)s * j.nchmax + chunk] = wg_total(wtot, NalCompose());
        __syncthreads();
    }
}

// is payload s there, and with which NAL unit type: an encoder context tells both by the device's own slice headers
__device__ __forceinline__ bool nal_present(const FerNalJob &j, int s, uint32_t len, int &type)
{
    if (j.hdr) {
        const uint32_t t = j.hdr[s * 4 + 3];
        type = t == 2u ? FERHIP_NAL_IDR : FERHIP_NAL_SLICE;
        return t != FER_PIC_ABSENT && len != 0u;
    }
    type = j.types[s] & 31;
    return true;
}

__global__ __launch_bounds__(64) void k_nal_plan(FerNalJob j)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    const uint32_t len = nal_len(j, s);
    int type;
    if (!nal_present(j, s, len, type)) {
        if (lane == 0) j.ent[s] = make_uint2(0u, 0u);
        return;
    }
    const uint32_t nch = (len + NAL_CHUNK - 1) / NAL_CHUNK;
    // a payload starts from counter 0: what comes into a chunk is the function in front of it at that state
    const uint4 tot = carry_scan(
        nch, lane, nal_identity(), NalCompose(), [&](uint32_t i) { return j.summ[(size_t)s * j.nchmax + i]; },
        [&](uint32_t i, const uint4 &in) { j.cin[(size_t)s * j.nchmax + i] = make_uint2(nal_out(in, 0u), nal_cnt(in, 0u)); });
    if (lane == 0) {
        const uint32_t ps = (j.ps && type == FERHIP_NAL_IDR) ? j.ps[(size_t)s * FER_NAL_PS_ROW + FER_NAL_PS_ROW - 1] : 0u;
        j.ent[s] = make_uint2(ps + 5u + len + nal_cnt(tot, 0u), (uint32_t)type);
    }
}

__global__ __launch_bounds__(64) void k_nal_index(FerNalJob j)
{
    const int lane = threadIdx.x;
    unsigned long long run = 0;
    uint32_t written = 0;
    for (int s0 = 0; s0 < j.n; s0 += 64) {
        const int s = s0 + lane;
        const uint2 e = s < j.n ? j.ent[s] : make_uint2(0u, 0u);
        const unsigned long long r = ((unsigned long long)e.x + 15ull) & ~15ull;
        const unsigned long long incl = wave_scan(r, lane, ScanAdd());
        const unsigned long long off = run + incl - r;
        if (s < j.n) {
            ferhip_au a;
            a.offset = off;
            a.bytes = e.x;
            a.nal_type = e.x ? (int32_t)e.y : 0;
            j.index[s] = a;
        }
        written += (uint32_t)__popcll(__ballot(e.x != 0u && off + r <= j.cap));
        run += __shfl(incl, 63);
    }
    if (lane == 0) {
        ferhip_au a;
        a.offset = run;
        a.bytes = written;
        a.nal_type = 0;
        j.index[j.n] = a;
    }
}

__global__ __launch_bounds__(NAL_THREADS) void k_nal_emit(FerNalJob j)
{
    const int s = blockIdx.y;
    const ferhip_au au = j.index[s];
    // no entry, or one whose 16-byte slots do not end within cap
    if (au.bytes == 0u || au.offset + (((unsigned long long)au.bytes + 15ull) & ~15ull) > j.cap) return;
    const uint32_t len = nal_len(j, s);
    const uint32_t nch = max((len + NAL_CHUNK - 1) / NAL_CHUNK, 1u);  // an empty payload still has its five prefix bytes
    const uint32_t pslen = (j.ps && au.nal_type == FERHIP_NAL_IDR) ? j.ps[(size_t)s * FER_NAL_PS_ROW + FER_NAL_PS_ROW - 1] : 0u;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __shared__ uint4 wtot[NAL_THREADS / 64];
    __shared__ __attribute__((aligned(16))) uint8_t img[NAL_IMG];
    for (uint32_t chunk = blockIdx.x; chunk < nch; chunk += gridDim.x) {
        int nvalid;
        const uint4 v = nal_load(j, s, len, chunk, tid, nvalid);
        const uint4 incl = wave_scan(nal_piece(v, nvalid), lane, NalCompose());
        wg_put(wtot, incl, wave, lane);
        uint4 excl = wave_excl(incl, lane, nal_identity());
        // chunk 0 starts from counter 0 with nothing inserted in front of it
        const uint2 cin = chunk ? j.cin[(size_t)s * j.nchmax + chunk] : make_uint2(0u, 0u);
        __syncthreads();
        const uint4 pre = wg_front(wtot, wave, nal_identity(), NalCompose());
        const uint4 tot = wg_total(wtot, NalCompose());
        excl = NalCompose()(pre, excl);
        // the chunk's span of the output: [a, a + n), staged in img at [sh, sh + n) so that 16-byte words line up
        const uint32_t head = chunk ? 0u : pslen + 5u;
        const unsigned long long a = au.offset + (chunk ? (unsigned long long)pslen + 5ull + (unsigned long long)chunk * NAL_CHUNK + cin.y : 0ull);
        const uint32_t sh = (uint32_t)a & 15u;
        const uint32_t nin = len > chunk * NAL_CHUNK ? min((uint32_t)NAL_CHUNK, len - chunk * NAL_CHUNK) : 0u;
        const uint32_t n = head + nin + nal_cnt(tot, cin.x);
        if (!chunk) {
            if ((uint32_t)tid < pslen) {
                const uint8_t *row = j.ps + (size_t)s * FER_NAL_PS_ROW;
                uint8_t b = row[tid];
                if (j.avcc) {  // the row's two start codes become the lengths of the SPS and the PPS unit
                    const uint32_t pps = row[FER_NAL_PS_ROW - 2];
                    if ((uint32_t)tid < 4u) b = (uint8_t)((pps - 4u) >> (8u * (3u - (uint32_t)tid)));
                    if ((uint32_t)tid >= pps && (uint32_t)tid < pps + 4u) b = (uint8_t)((pslen - pps - 4u) >> (8u * (3u - ((uint32_t)tid - pps))));
                }
                img[tid] = b;
            }
            if ((uint32_t)tid >= pslen && (uint32_t)tid < pslen + 5u) {
                const uint32_t k = (uint32_t)tid - pslen;
                const uint32_t ulen = au.bytes - pslen - 4u;  // header byte + escaped payload
                const uint8_t pre = j.avcc ? (uint8_t)(ulen >> (8u * (3u - k))) : (uint8_t)(k == 3u);
                img[tid] = k < 4u ? pre : (uint8_t)(1u << 5 | ((uint32_t)au.nal_type & 31u));
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
        store_span<NAL_THREADS>(j.dst + (a - sh), img, sh, sh + n);  // the entry's slots end within cap (above): nothing to cut
        __syncthreads();
    }
}
void fer_launch_nal_count(const FerNalJob &j, hipStream_t st)
{
    hipLaunchKernelGGL(k_nal_count, dim3(nal_grid_x(j), j.n), dim3(NAL_THREADS), 0, st, j);
    hipLaunchKernelGGL(k_nal_plan, dim3(j.n), dim3(64), 0, st, j);
}

// count + plan: fills j.index (device) for the payloads of j; nothing of dst is touched
static void fer_launch_nal_plan(const FerNalJob &j, hipStream_t st)
{
    fer_launch_nal_count(j, st);
    hipLaunchKernelGGL(k_nal_index, dim3(1), dim3(64), 0, st, j);
}

// writes every entry of j.index whose 16-byte slots end within j.cap
static void fer_launch_nal_emit(const FerNalJob &j, hipStream_t st)
{
    hipLaunchKernelGGL(k_nal_emit, dim3(nal_grid_x(j), j.n), dim3(NAL_THREADS), 0, st, j);
}

// ---- host side: an encoder context's buffers, allocated on first use
static int nal_alloc(ferhip_ctx *c)
{
    if (c->nal_nchmax) return 0;
    FerDev &d = c->d;
    const int nchmax = (int)((d.bits_cap_words * 4 + 4095) / 4096);
    // the allocators keep what exists: a call after a failed one allocates only what is still missing
    if (dalloc(c, &c->nal_summ, (size_t)d.S * nchmax) || dalloc(c, &c->nal_cin, (size_t)d.S * nchmax) || dalloc(c, &c->nal_ent, (size_t)d.S) ||
        dalloc(c, &c->nal_index, (size_t)d.S + 1) || halloc(c, &c->h_nal_index, (size_t)d.S + 1) ||
        hipDeviceSynchronize() != hipSuccess) {  // dalloc clears on the null stream
        (void)hipGetLastError();
        fprintf(stderr, "ferhip: could not allocate the NAL framing buffers\n");
        return FERHIP_E_HIP;
    }
    c->nal_nchmax = nchmax;
    return 0;
}

// FERHIP_AU_PARAM_SETS: the framed SPS + PPS of every stream in the device table.  Rows that can have changed are built
// into the next slot of a pinned ring and sent from there on the context's stream.
static int ps_refresh(ferhip_ctx *c, bool avcc)
{
    const int S = c->d.S;
    if (c->ps_dirty.empty()) {
        if (dalloc(c, &c->d_ps, (size_t)S * FER_NAL_PS_ROW) || hipDeviceSynchronize() != hipSuccess ||  // as in nal_alloc
            c->ps_ring.create((size_t)S * FER_NAL_PS_ROW)) {
            (void)hipGetLastError();
            return FERHIP_E_HIP;
        }
        c->ps_dirty.assign(S, 1);
    }
    bool any = false;
    for (int s = 0; s < S; s++) any |= c->ps_dirty[s] != 0;
    if (!any) return (avcc && c->ps_wide) ? FERHIP_E_UNSUP : 0;
    uint8_t *slot = (uint8_t *)c->ps_ring.next();
    if (!slot) return FERHIP_E_HIP;
    for (int s = 0; s < S; s++) {
        if (!c->ps_dirty[s]) continue;
        uint8_t rbsp[64], nal[2 * (5 + 96)];
        size_t n = ferhip_write_sps(c, rbsp, sizeof rbsp);
        size_t m = ferhip_write_nal(1, 7, rbsp, n, nal);
        const size_t pps_at = m;
        n = ferhip_write_pps_stream(c, s, rbsp, sizeof rbsp);
        m += ferhip_write_nal(1, 8, rbsp, n, nal + m);
        if (m > FER_NAL_PS_ROW - 1) return FERHIP_E_UNSUP;
        uint8_t *row = slot + (size_t)s * FER_NAL_PS_ROW;
        memset(row, 0, FER_NAL_PS_ROW);
        memcpy(row, nal, m);
        row[FER_NAL_PS_ROW - 1] = (uint8_t)m;
        if (m <= FER_NAL_PS_ROW - 2)
            row[FER_NAL_PS_ROW - 2] = (uint8_t)pps_at;
        else
            c->ps_wide = true;  // a row without room for the record: such a context has no length-prefixed form
    }
    for (int s = 0; s < S;) {  // one copy per run of rows
        if (!c->ps_dirty[s]) {
            s++;
            continue;
        }
        int e = s;
        while (e < S && c->ps_dirty[e]) c->ps_dirty[e++] = 0;
        CK(hipMemcpyAsync(c->d_ps + (size_t)s * FER_NAL_PS_ROW, slot + (size_t)s * FER_NAL_PS_ROW, (size_t)(e - s) * FER_NAL_PS_ROW,
                          hipMemcpyHostToDevice, c->st));
        s = e;
    }
    if (int rc = c->ps_ring.sent(c->st)) return rc;
    return (avcc && c->ps_wide) ? FERHIP_E_UNSUP : 0;
}

int fer_nal_prepare(ferhip_ctx *c, int flags, FerNalJob &j)
{
    if (!c->nal_ready) return FERHIP_E_STATE;
    (void)hipSetDevice(c->device);
    if (nal_alloc(c)) return FERHIP_E_HIP;
    if (flags & FERHIP_AU_PARAM_SETS) {
        int rc = ps_refresh(c, (flags & FERHIP_AU_AVCC) != 0);
        if (rc) return rc;
    }
    FerDev &d = c->d;
    j.src = (const uint8_t *)d.bits;
    j.src_stride = d.bits_cap_words * 4;
    j.lens = d.out_bytes;
    j.hdr = d.hdr;
    j.types = nullptr;
    j.ps = (flags & FERHIP_AU_PARAM_SETS) ? c->d_ps : nullptr;
    j.avcc = (flags & FERHIP_AU_AVCC) ? 1 : 0;
    j.n = d.S;
    j.nchmax = c->nal_nchmax;
    j.summ = c->nal_summ;
    j.cin = c->nal_cin;
    j.ent = c->nal_ent;
    j.index = c->nal_index;
    j.dst = nullptr;
    j.cap = 0;
    return 0;
}

extern "C" int ferhip_pack_nal(ferhip_ctx *c, int flags, void *d_dst, size_t cap, ferhip_au *d_index)
{
    if (!c || !d_index || (flags & ~(FERHIP_AU_PARAM_SETS | FERHIP_AU_AVCC)) || ((uintptr_t)d_dst & 15) || ((uintptr_t)d_index & 7) || (!d_dst && cap))
        return FERHIP_E_ARG;
    FerNalJob j;
    int rc = fer_nal_prepare(c, flags, j);
    if (rc) return rc;
    j.index = d_index;
    j.dst = (uint8_t *)d_dst;
    j.cap = cap;
    fer_launch_nal_plan(j, c->st);
    fer_launch_nal_emit(j, c->st);
    CK(hipGetLastError());
    return 0;
}

extern "C" int ferhip_fetch_nal(ferhip_ctx *c, int flags, void *h_dst, size_t cap, ferhip_au *h_index)
{
    if (!c || !h_index || (flags & ~(FERHIP_AU_PARAM_SETS | FERHIP_AU_AVCC)) || (!h_dst && cap)) return FERHIP_E_ARG;
    FerNalJob j;
    int rc = fer_nal_prepare(c, flags, j);
    if (rc) return rc;
    const int S = c->d.S;
    j.cap = cap;
    fer_launch_nal_plan(j, c->st);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(c->h_nal_index, c->nal_index, sizeof(ferhip_au) * (S + 1), hipMemcpyDeviceToHost, c->st));
    CK(hipStreamSynchronize(c->st));
    memcpy(h_index, c->h_nal_index, sizeof(ferhip_au) * (S + 1));
    const size_t total = (size_t)c->h_nal_index[S].offset;
    if (total > cap) return FERHIP_E_ARG;
    if (total == 0) return 0;
    if (c->nal_buf_cap < total) {
        if (c->nal_buf) CK(hipFree(c->nal_buf));
        c->nal_buf = nullptr;
        c->nal_buf_cap = 0;
        const size_t want = (total + total / 4 + 65535) & ~(size_t)65535;
        CK(hipMalloc((void **)&c->nal_buf, want));
        CK(hipMemsetAsync(c->nal_buf, 0, want, c->st));  // the bytes between entries are copied out too
        c->nal_buf_cap = want;
    }
    j.dst = c->nal_buf;
    j.cap = total;
    fer_launch_nal_emit(j, c->st);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(h_dst, c->nal_buf, total, hipMemcpyDeviceToHost, c->st));
    CK(hipStreamSynchronize(c->st));
    return 0;
}

// known-answer surface: host payloads through the same kernels, on the null stream with buffers of its own
static int frame_nal_blocks(const uint8_t *payloads, size_t stride, const uint32_t *lens, const int32_t *nal_type, size_t n, int flags,
                            uint8_t *out, size_t cap, ferhip_au *index)
{
    if ((flags & ~FERHIP_AU_AVCC) || !lens || !nal_type || !index || n == 0 || n > 65535 || (!out && cap)) return FERHIP_E_ARG;
    uint32_t maxlen = 0;
    for (size_t i = 0; i < n; i++) {
        if (lens[i] > stride || (lens[i] && !payloads)) return FERHIP_E_ARG;
        maxlen = std::max(maxlen, lens[i]);
    }
    const size_t pitch = std::max<size_t>(((size_t)maxlen + 15) & ~(size_t)15, 16);
    const int nchmax = (int)std::max<size_t>(((size_t)maxlen + 4095) / 4096, 1);
    DevBuf<uint8_t> src, dst;
    DevBuf<uint32_t> dl;
    DevBuf<int32_t> dt;
    DevBuf<uint4> summ;
    DevBuf<uint2> cin, ent;
    DevBuf<ferhip_au> idx;
    if (src.reserve(pitch * n) || dst.reserve(std::max<size_t>(cap, 16)) || dl.reserve(n) || dt.reserve(n) || summ.reserve(n * nchmax) ||
        cin.reserve(n * nchmax) || ent.reserve(n) || idx.reserve(n + 1))
        return FERHIP_E_HIP;
    CK(hipMemset(src, 0, pitch * n));
    if (maxlen) CK(hipMemcpy2D(src, pitch, payloads, stride, maxlen, n, hipMemcpyHostToDevice));
    CK(hipMemcpy(dl, lens, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(dt, nal_type, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    if (cap) CK(hipMemcpy(dst, out, cap, hipMemcpyHostToDevice));
    FerNalJob j;
    j.src = src;
    j.src_stride = pitch;
    j.lens = dl;
    j.hdr = nullptr;
    j.types = dt;
    j.ps = nullptr;
    j.avcc = (flags & FERHIP_AU_AVCC) ? 1 : 0;
    j.n = (int)n;
    j.nchmax = nchmax;
    j.summ = summ;
    j.cin = cin;
    j.ent = ent;
    j.index = idx;
    j.dst = dst;
    j.cap = cap;
    fer_launch_nal_plan(j, nullptr);
    fer_launch_nal_emit(j, nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    if (cap) CK(hipMemcpy(out, dst, cap, hipMemcpyDeviceToHost));
    CK(hipMemcpy(index, idx, sizeof(ferhip_au) * (n + 1), hipMemcpyDeviceToHost));
    return 0;  // the temporaries go with their owners
}

extern "C" int ferhip_frame_nal_blocks(const uint8_t *payloads, size_t stride, const uint32_t *lens, const int32_t *nal_type,
                                       size_t n, uint8_t *out, size_t cap, ferhip_au *index)
{
    return frame_nal_blocks(payloads, stride, lens, nal_type, n, 0, out, cap, index);
}

extern "C" int ferhip_frame_nal_blocks_fmt(const uint8_t *payloads, size_t stride, const uint32_t *lens, const int32_t *nal_type,
                                           size_t n, int flags, uint8_t *out, size_t cap, ferhip_au *index)
{
    return frame_nal_blocks(payloads, stride, lens, nal_type, n, flags, out, cap, index);
}

// AVCDecoderConfigurationRecord (ISO/IEC 14496-15 5.2.4.1) of stream s: one SPS and the stream's own PPS, 4-byte lengths
extern "C" size_t ferhip_write_avcc_config(ferhip_ctx *c, int s, uint8_t *out, size_t cap)
{
    if (!c || !out || s < 0 || s >= c->d.S) return 0;
    uint8_t rbsp[64], sps[2 * (5 + 96)], pps[2 * (5 + 96)];
    size_t n = ferhip_write_sps(c, rbsp, sizeof rbsp);
    if (n < 3) return 0;
    const uint8_t prof[3] = {rbsp[0], rbsp[1], rbsp[2]};
    const size_t ns = ferhip_write_nal(1, 7, rbsp, n, sps) - 4;  // the unit behind its start code
    n = ferhip_write_pps_stream(c, s, rbsp, sizeof rbsp);
    if (n == 0) return 0;
    const size_t np = ferhip_write_nal(1, 8, rbsp, n, pps) - 4;
    const size_t total = 6 + 2 + ns + 1 + 2 + np;
    if (total > cap || ns > 65535 || np > 65535) return 0;
    uint8_t *w = out;
    *w++ = 1;  // configurationVersion
    *w++ = prof[0];
    *w++ = prof[1];
    *w++ = prof[2];
    *w++ = 0xFC | 3;  // lengthSizeMinusOne
    *w++ = 0xE0 | 1;  // numOfSequenceParameterSets
    *w++ = (uint8_t)(ns >> 8);
    *w++ = (uint8_t)ns;
    memcpy(w, sps + 4, ns);
    w += ns;
    *w++ = 1;  // numOfPictureParameterSets
    *w++ = (uint8_t)(np >> 8);
    *w++ = (uint8_t)np;
    memcpy(w, pps + 4, np);
    w += np;
    return (size_t)(w - out);
}
