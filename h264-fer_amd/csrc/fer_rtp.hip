// fer_rtp.hip -- the coded pictures as RTP packets of RFC 6184, packetization-mode 1, on the device (ferhip_pack_rtp,
// ferhip_fetch_rtp, ferhip_rtp_blocks; the definition stands in include/ferhip.h): one STAP-A packet for the parameter
// sets, a single-NAL packet for a unit that fits, FU-A fragments for one that does not, every packet behind its 12-byte RTP
// header at a multiple of 16, with a table of (offset, bytes, stream) and an index per stream.
//
// The unit that is cut into packets is the escaped one, so the emulation prevention comes first, and it is fer_nalpack.hip's:
//   k_nal_count, k_nal_plan   run as they are (fer_launch_nal_count): every 4096-byte chunk's incoming counter and the 03
//                bytes in front of it, and the unit's size N.
//   k_rtp_index  one wavefront: a lane takes a stream, derives its packet count and the sum of its packets' 16-rounded
//                sizes from N, and the exclusive sums over the streams of both give the index.
//   k_rtp_emit   grid (chunk, stream): the scan of k_nal_emit gives every lane its position e in the escaped payload; byte
//                e goes to packet e / F at byte 14 + e % F (one packet at byte 13 + e for a unit that fits), and the packets
//                of a stream lie one pitch = P rounded up to 16 apart, so the chunk's output is placed in LDS in output
//                coordinates.  The chunk also fills the header bytes and the table row of every packet that begins in it.
//                A 16-byte word of the image lies within one packet (pitch and offsets are multiples of 16): a word the
//                chunk fills goes out whole, the others byte-wise, masked to the bytes of the packet that are the chunk's.
//                Chunk 0 also places the STAP-A packet from the parameter set table.
// No workgroup waits for another one: the phases are separate launches on one stream.
// The host side follows the kernels; the SDP format parameters (ferhip_write_sdp_fmtp) stand at the end of the file.
#include "fer_nal.h"
#include "fer_nalsplit.h"
#include <string.h>
#include <algorithm>

struct FerRtpJob {
    FerNalJob nal;           // ps = null, index / dst unused: the units are counted without their parameter sets
    const uint8_t *ps;       // [n][FER_NAL_PS_ROW] or null: the STAP-A packet in front of an IDR slice
    const uint32_t *hdr;     // [n][3] ferhip_rtp_hdr: ssrc, timestamp, seq | payload_type << 16
    uint32_t P;              // max_packet
    uint8_t *dst;
    unsigned long long cap;
    ferhip_rtp_pkt *pkts;
    unsigned long long pkts_cap;
    ferhip_rtp_au *index;    // [n + 1] device
};

// The packets of one stream's access unit, from the size of its slice unit and of its parameter set row
struct RtpPlan {
    uint32_t hl;      // bytes in front of the escaped payload in a slice packet: 12 + 1 (single NAL) or 12 + 2 (FU-A)
    uint32_t F;       // escaped payload bytes per slice packet; a single-NAL packet takes them all
    uint32_t n;       // slice packets
    uint32_t npay;    // escaped payload bytes = N - 1
    uint32_t pitch;   // distance of the slice packets
    uint32_t stap;    // bytes of the STAP-A packet, 0 = none
    __device__ __forceinline__ uint32_t pkt_bytes(uint32_t k) const { return hl + min(F, npay - k * F); }
    __device__ __forceinline__ uint32_t stap_slot() const { return (stap + 15u) & ~15u; }
    __device__ __forceinline__ unsigned long long slots() const
    {
        return (unsigned long long)stap_slot() + (unsigned long long)(n - 1u) * pitch + ((pkt_bytes(n - 1u) + 15u) & ~15u);
    }
};

// ent = k_nal_plan's (5 + payload + 03 bytes, type) of a stream that is there
__device__ __forceinline__ RtpPlan rtp_plan(const FerRtpJob &j, int s, const uint2 &ent)
{
    RtpPlan p;
    const uint32_t N = ent.x - 4u, B = j.P - 12u;
    const bool fu = N > B;
    p.npay = N - 1u;
    p.hl = fu ? 14u : 13u;
    p.F = fu ? B - 2u : 0xffffffffu;
    p.n = fu ? (p.npay + p.F - 1u) / p.F : 1u;
    p.pitch = (j.P + 15u) & ~15u;
    const uint32_t pslen = (j.ps && ent.y == (uint32_t)FERHIP_NAL_IDR) ? j.ps[(size_t)s * FER_NAL_PS_ROW + FER_NAL_PS_ROW - 1] : 0u;
    p.stap = pslen ? pslen + 9u : 0u;  // 12 + 1 + two sizes of 2 bytes in place of two start codes of 4
    return p;
}

__global__ __launch_bounds__(64) void k_rtp_index(FerRtpJob j)
{
    const int lane = threadIdx.x, n = j.nal.n;
    unsigned long long run = 0, prun = 0;
    uint32_t written = 0;
    for (int s0 = 0; s0 < n; s0 += 64) {
        const int s = s0 + lane;
        const uint2 e = s < n ? j.nal.ent[s] : make_uint2(0u, 0u);
        unsigned long long r = 0, np = 0;
        if (e.x) {
            const RtpPlan p = rtp_plan(j, s, e);
            r = p.slots();
            np = p.n + (p.stap ? 1u : 0u);
        }
        const unsigned long long incl = wave_scan(r, lane, ScanAdd()), pincl = wave_scan(np, lane, ScanAdd());
        const unsigned long long off = run + incl - r, first = prun + pincl - np;
        if (s < n) {
            ferhip_rtp_au a;
            a.offset = e.x ? off : 0ull;
            a.bytes = (uint32_t)r;
            a.nal_type = e.x ? (int32_t)e.y : 0;
            a.first_pkt = e.x ? (uint32_t)first : 0u;
            a.npkts = (uint32_t)np;
            j.index[s] = a;
        }
        written += (uint32_t)__popcll(__ballot(e.x != 0u && off + r <= j.cap && first + np <= j.pkts_cap));
        run += __shfl(incl, 63);
        prun += __shfl(pincl, 63);
    }
    if (lane == 0) {
        ferhip_rtp_au a;
        a.offset = run;
        a.bytes = written;
        a.nal_type = 0;
        a.first_pkt = (uint32_t)prun;
        a.npkts = 0u;
        j.index[n] = a;
    }
}

// LDS image of one chunk's output.  A chunk holds at most NAL_CHUNK + NAL_CHUNK / 2 + 1 = 6145 escaped bytes.  They begin
// anywhere in a packet, so they touch at most (F - 1 + 6144) / F + 1 packets, and every step to the next packet adds
// pitch - F <= 14 + 15 bytes (the next packet's 14 header bytes and the rounding to 16); in front stand up to 14 header
// bytes and up to 15 bytes of misalignment.  F >= 66 (P >= 80): 6145 + 14 + 15 + 29 * (6143 / 66 + 1) = 8900.  (At P = 80
// itself a step adds 14 bytes: 7490, under 8 KB; P = 81 with pitch 96 is the worst case, 8842.)
#define RTP_IMG ((NAL_CHUNK + NAL_CHUNK / 2 + 1 + 14 + 15 + 29 * ((NAL_CHUNK + NAL_CHUNK / 2 - 1) / 66 + 1) + 15) & ~15)
#define RTP_STAP ((FER_NAL_PS_ROW + 9 + 15) & ~15)

// byte b < hl of slice packet k of a stream: RTP header, then the unit's header byte or the FU indicator and FU header
__device__ __forceinline__ uint8_t rtp_hdr_byte(const RtpPlan &p, uint32_t k, uint32_t b, uint32_t h, uint32_t ssrc, uint32_t ts,
                                                uint32_t seq0, uint32_t pt)
{
    const bool last = k == p.n - 1u;
    const uint32_t seq = seq0 + (p.stap ? 1u : 0u) + k;
    switch (b) {
    case 0: return 0x80;
    case 1: return (uint8_t)((last ? 0x80u : 0u) | pt);
    case 2: return (uint8_t)(seq >> 8);
    case 3: return (uint8_t)seq;
    case 4: case 5: case 6: case 7: return (uint8_t)(ts >> (8u * (7u - b)));
    case 8: case 9: case 10: case 11: return (uint8_t)(ssrc >> (8u * (11u - b)));
    case 12: return (uint8_t)(p.hl == 13u ? h : ((h & 0xE0u) | 28u));
    default: return (uint8_t)((k == 0u ? 0x80u : 0u) | (last ? 0x40u : 0u) | (h & 0x1Fu));
    }
}

__global__ __launch_bounds__(NAL_THREADS) void k_rtp_emit(FerRtpJob j)
{
    const int s = blockIdx.y;
    const ferhip_rtp_au au = j.index[s];
    // no picture, or packets or table rows that do not end within their caps
    if (au.npkts == 0u || au.offset + au.bytes > j.cap || (unsigned long long)au.first_pkt + au.npkts > j.pkts_cap) return;
    const uint2 ent = j.nal.ent[s];
    const RtpPlan p = rtp_plan(j, s, ent);
    const uint32_t h = 1u << 5 | (ent.y & 31u);
    const uint32_t ssrc = j.hdr[s * 3], ts = j.hdr[s * 3 + 1], seq0 = j.hdr[s * 3 + 2] & 0xffffu, pt = (j.hdr[s * 3 + 2] >> 16) & 0x7fu;
    const unsigned long long sbase = au.offset + p.stap_slot();  // where the slice packets begin
    const uint32_t row0 = au.first_pkt + (p.stap ? 1u : 0u);
    const uint32_t len = nal_len(j.nal, s);
    const uint32_t nch = max((len + NAL_CHUNK - 1) / NAL_CHUNK, 1u);  // an empty payload still has its header byte
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __shared__ uint4 wtot[NAL_THREADS / 64];
    __shared__ __attribute__((aligned(16))) uint8_t img[RTP_IMG];
    __shared__ __attribute__((aligned(16))) uint8_t stap[RTP_STAP];
    __shared__ uint32_t pps_at;

    if (blockIdx.x == 0 && p.stap) {
        // the row is 00 00 00 01 SPS 00 00 00 01 PPS: byte i of the SPS lands at i + 11, byte i of the PPS at i + 9, and the
        // PPS's size where the last two bytes of its start code would land
        const uint8_t *row = j.ps + (size_t)s * FER_NAL_PS_ROW;
        // where the PPS's start code begins: the second 00 00 00 01 of the row (escaped units hold none, and an SPS ends on
        // a non-zero byte); a row of FER_NAL_PS_ROW - 1 bytes has no room to record it
        const uint32_t m = p.stap - 9u;
        if (tid == 0) pps_at = m;
        __syncthreads();
        if ((uint32_t)tid >= 5u && (uint32_t)tid + 4u <= m && row[tid] == 0 && row[tid + 1] == 0 && row[tid + 2] == 0 && row[tid + 3] == 1)
            atomicMin(&pps_at, (uint32_t)tid);
        __syncthreads();
        const uint32_t pps = pps_at;
        const uint32_t ns = pps - 4u, np = m - pps - 4u;
        const uint32_t t = (uint32_t)tid;
        if (t < p.stap) {
            uint8_t b;
            if (t < 12u) {
                b = t == 0u ? 0x80 : t == 1u ? (uint8_t)pt : t == 2u ? (uint8_t)(seq0 >> 8) : t == 3u ? (uint8_t)seq0
                    : t < 8u ? (uint8_t)(ts >> (8u * (7u - t))) : (uint8_t)(ssrc >> (8u * (11u - t)));
            } else if (t == 12u)
                b = 0x20 | 24;
            else if (t < 15u)
                b = (uint8_t)(ns >> (8u * (14u - t)));
            else if (t < 15u + ns)
                b = row[t - 11u];
            else if (t < 17u + ns)
                b = (uint8_t)(np >> (8u * (16u + ns - t)));
            else
                b = row[t - 9u];
            stap[t] = b;
        }
        __syncthreads();
        store_span<NAL_THREADS>(j.dst + au.offset, stap, 0u, p.stap);
        if (tid == 0) {
            ferhip_rtp_pkt r;
            r.offset = au.offset;
            r.bytes = p.stap;
            r.stream = (uint32_t)s;
            j.pkts[au.first_pkt] = r;
        }
    }

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
        // the chunk's escaped bytes [e0, e1) of the payload lie in packets [k0, ke); it begins packets [kb, ke)
        const uint32_t nin = len > chunk * NAL_CHUNK ? min((uint32_t)NAL_CHUNK, len - chunk * NAL_CHUNK) : 0u;
        const uint32_t e0 = chunk * NAL_CHUNK + cin.y, e1 = e0 + nin + nal_cnt(tot, cin.x);
        const uint32_t k0 = e0 / p.F, w0 = e0 - k0 * p.F;
        const uint32_t kb = w0 ? k0 + 1u : k0;
        const uint32_t ke = (e1 > e0 ? (e1 - 1u) / p.F : k0) + 1u;  // an empty payload: chunk 0 begins packet 0
        // image coordinates: bytes from the first slice packet's start, less r0 rounded down to 16
        const uint32_t r0 = k0 * p.pitch + (w0 ? p.hl + w0 : 0u), rbase = r0 & ~15u;
        for (uint32_t t = (uint32_t)tid; t < (ke - kb) * 16u; t += NAL_THREADS) {
            const uint32_t k = kb + (t >> 4), b = t & 15u;
            if (b < p.hl) img[k * p.pitch + b - rbase] = rtp_hdr_byte(p, k, b, h, ssrc, ts, seq0, pt);
        }
        {
            uint32_t z = nal_out(excl, cin.x);
            const uint32_t e = e0 + (uint32_t)tid * 16u + nal_cnt(excl, cin.x);
            const uint32_t k = e / p.F;
            uint32_t w = e - k * p.F;
            uint32_t q = k * p.pitch + p.hl + w - rbase;
            const uint32_t step = p.pitch - p.F;  // from a packet's last payload byte to the next one's first, less one
#define RTP_PUT(x)                 \
    {                              \
        img[q++] = (uint8_t)(x);   \
        if (++w == p.F) {          \
            w = 0u;                \
            q += step;             \
        }                          \
    }
#define NAL_DWORD(wd, kk)                                  \
    _Pragma("unroll") for (int qq = 0; qq < 4; qq++)       \
    {                                                      \
        if (4 * (kk) + qq < nvalid) {                      \
            const uint32_t b = ((wd) >> (8 * qq)) & 0xffu; \
            if (nal_step(b, z)) RTP_PUT(3)                 \
            RTP_PUT(b)                                     \
        }                                                  \
    }
            NAL_DWORD(v.x, 0)
            NAL_DWORD(v.y, 1)
            NAL_DWORD(v.z, 2)
            NAL_DWORD(v.w, 3)
#undef NAL_DWORD
#undef RTP_PUT
        }
        __syncthreads();
        // the image ends with the last packet's last byte; word i covers bytes [o, o + 16) of packet k, of which the chunk
        // owns [lo, hi): from its first byte (or the packet's start, if the packet begins here) to its last
        const uint32_t rend = (ke - 1u) * p.pitch + p.hl + min(p.F, e1 - (ke - 1u) * p.F);
        uint8_t *dst16 = j.dst + sbase + rbase;
        for (uint32_t i = (uint32_t)tid; i < (rend - rbase + 15u) >> 4; i += NAL_THREADS) {
            const uint32_t r = rbase + (i << 4), k = r / p.pitch, o = r - k * p.pitch;
            const uint32_t a = (k == k0 && w0) ? p.hl + w0 : 0u;
            const uint32_t b = p.hl + min(p.F, e1 - k * p.F);
            const uint32_t lo = max(o, a), hi = min(o + 16u, b);
            if (lo == o && hi == o + 16u) {
                *(uint4 *)(dst16 + (i << 4)) = *(const uint4 *)(img + (i << 4));
            } else {
                for (uint32_t x = lo; x < hi; x++) dst16[(i << 4) + x - o] = img[(i << 4) + x - o];
            }
        }
        for (uint32_t t = (uint32_t)tid; t < ke - kb; t += NAL_THREADS) {
            const uint32_t k = kb + t;
            ferhip_rtp_pkt r;
            r.offset = sbase + (unsigned long long)k * p.pitch;
            r.bytes = p.pkt_bytes(k);
            r.stream = (uint32_t)s;
            j.pkts[row0 + k] = r;
        }
        __syncthreads();
    }
}

static void rtp_launch_plan(const FerRtpJob &j, hipStream_t st)
{
    fer_launch_nal_count(j.nal, st);
    hipLaunchKernelGGL(k_rtp_index, dim3(1), dim3(64), 0, st, j);
}

static void rtp_launch_emit(const FerRtpJob &j, hipStream_t st)
{
    hipLaunchKernelGGL(k_rtp_emit, dim3(nal_grid_x(j.nal), j.nal.n), dim3(NAL_THREADS), 0, st, j);
}

static bool rtp_args_ok(int flags, int max_packet, const ferhip_rtp_hdr *hdr, size_t n)
{
    if ((flags & ~FERHIP_AU_PARAM_SETS) || max_packet < 80 || max_packet > 65535 || !hdr) return false;
    for (size_t s = 0; s < n; s++)
        if (hdr[s].payload_type > 127 || hdr[s].reserved != 0) return false;
    return true;
}

// ---- host side: an encoder context's buffers, allocated on first use; hdr[] goes through the next slot of a pinned ring
static int rtp_prepare(ferhip_ctx *c, int flags, int max_packet, const ferhip_rtp_hdr *hdr, FerRtpJob &j)
{
    static_assert(sizeof(ferhip_rtp_hdr) == 12 && sizeof(ferhip_rtp_pkt) == 16 && sizeof(ferhip_rtp_au) == 24, "ABI");
    int rc = fer_nal_prepare(c, flags, j.nal);
    if (rc) return rc;
    const int S = c->d.S;
    if (!c->rtp_ready) {  // dalloc, halloc and the ring keep what exists: a call after a failed one allocates what is missing
        if (dalloc(c, &c->rtp_index, (size_t)S + 1) || halloc(c, &c->h_rtp_index, (size_t)S + 1) || dalloc(c, &c->d_rtp_hdr, (size_t)S * 3) ||
            hipDeviceSynchronize() != hipSuccess ||  // dalloc clears on the null stream
            c->rtp_ring.create((size_t)S * sizeof(ferhip_rtp_hdr))) {
            (void)hipGetLastError();
            fprintf(stderr, "ferhip: could not allocate the RTP buffers\n");
            return FERHIP_E_HIP;
        }
        c->rtp_ready = true;
    }
    void *slot = c->rtp_ring.next();
    if (!slot) return FERHIP_E_HIP;
    memcpy(slot, hdr, (size_t)S * sizeof(ferhip_rtp_hdr));
    CK(hipMemcpyAsync(c->d_rtp_hdr, slot, (size_t)S * sizeof(ferhip_rtp_hdr), hipMemcpyHostToDevice, c->st));
    if ((rc = c->rtp_ring.sent(c->st))) return rc;
    j.ps = j.nal.ps;
    j.nal.ps = nullptr;
    j.nal.avcc = 0;
    j.hdr = c->d_rtp_hdr;
    j.P = (uint32_t)max_packet;
    j.dst = nullptr;
    j.cap = 0;
    j.pkts = nullptr;
    j.pkts_cap = 0;
    j.index = c->rtp_index;
    return 0;
}

extern "C" int ferhip_pack_rtp(ferhip_ctx *c, int flags, int max_packet, const ferhip_rtp_hdr *hdr, void *d_dst, size_t cap,
                               ferhip_rtp_pkt *d_pkts, size_t pkts_cap, ferhip_rtp_au *d_index)
{
    if (!c || !d_index || !rtp_args_ok(flags, max_packet, hdr, (size_t)c->d.S) || ((uintptr_t)d_dst & 15) || ((uintptr_t)d_pkts & 7) ||
        ((uintptr_t)d_index & 7) || (!d_dst && cap) || (!d_pkts && pkts_cap))
        return FERHIP_E_ARG;
    FerRtpJob j;
    int rc = rtp_prepare(c, flags, max_packet, hdr, j);
    if (rc) return rc;
    j.index = d_index;
    j.dst = (uint8_t *)d_dst;
    j.cap = cap;
    j.pkts = d_pkts;
    j.pkts_cap = pkts_cap;
    rtp_launch_plan(j, c->st);
    rtp_launch_emit(j, c->st);
    CK(hipGetLastError());
    return 0;
}

extern "C" int ferhip_fetch_rtp(ferhip_ctx *c, int flags, int max_packet, const ferhip_rtp_hdr *hdr, void *h_dst, size_t cap,
                                ferhip_rtp_pkt *h_pkts, size_t pkts_cap, ferhip_rtp_au *h_index)
{
    if (!c || !h_index || !rtp_args_ok(flags, max_packet, hdr, (size_t)c->d.S) || (!h_dst && cap) || (!h_pkts && pkts_cap)) return FERHIP_E_ARG;
    FerRtpJob j;
    int rc = rtp_prepare(c, flags, max_packet, hdr, j);
    if (rc) return rc;
    const int S = c->d.S;
    j.cap = cap;
    j.pkts_cap = pkts_cap;
    rtp_launch_plan(j, c->st);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(c->h_rtp_index, c->rtp_index, sizeof(ferhip_rtp_au) * (S + 1), hipMemcpyDeviceToHost, c->st));
    CK(hipStreamSynchronize(c->st));
    memcpy(h_index, c->h_rtp_index, sizeof(ferhip_rtp_au) * (S + 1));
    const size_t total = (size_t)c->h_rtp_index[S].offset, npk = c->h_rtp_index[S].first_pkt;
    if (total > cap || npk > pkts_cap) return FERHIP_E_ARG;
    if (total == 0) return 0;
    if (c->rtp_buf.cap < total) {
        const size_t want = (total + total / 4 + 65535) & ~(size_t)65535;
        if (c->rtp_buf.reserve(total, want)) return FERHIP_E_HIP;
        CK(hipMemsetAsync(c->rtp_buf, 0, want, c->st));  // the bytes between packets are copied out too
    }
    if (c->rtp_pkts.reserve(npk, npk + npk / 4 + 256)) return FERHIP_E_HIP;
    j.dst = c->rtp_buf;
    j.cap = total;
    j.pkts = c->rtp_pkts;
    j.pkts_cap = npk;
    rtp_launch_emit(j, c->st);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(h_dst, c->rtp_buf, total, hipMemcpyDeviceToHost, c->st));
    CK(hipMemcpyAsync(h_pkts, c->rtp_pkts, sizeof(ferhip_rtp_pkt) * npk, hipMemcpyDeviceToHost, c->st));
    CK(hipStreamSynchronize(c->st));
    return 0;
}

// known-answer surface: host payloads through the same kernels, on the null stream with buffers of its own
extern "C" int ferhip_rtp_blocks(const uint8_t *payloads, size_t stride, const uint32_t *lens, const int32_t *nal_type, size_t n,
                                 int max_packet, const ferhip_rtp_hdr *hdr, uint8_t *out, size_t cap, ferhip_rtp_pkt *pkts,
                                 size_t pkts_cap, ferhip_rtp_au *index)
{
    if (!lens || !nal_type || !index || n == 0 || n > 65535 || !rtp_args_ok(0, max_packet, hdr, n) || (!out && cap) || (!pkts && pkts_cap))
        return FERHIP_E_ARG;
    uint32_t maxlen = 0;
    for (size_t i = 0; i < n; i++) {
        if (lens[i] > stride || lens[i] > (1u << 30) || (lens[i] && !payloads)) return FERHIP_E_ARG;
        maxlen = std::max(maxlen, lens[i]);
    }
    const size_t pitch = std::max<size_t>(((size_t)maxlen + 15) & ~(size_t)15, 16);
    const int nchmax = (int)std::max<size_t>(((size_t)maxlen + 4095) / 4096, 1);
    DevBuf<uint8_t> src, dst;
    DevBuf<uint32_t> dl, dh;
    DevBuf<int32_t> dt;
    DevBuf<uint4> summ;
    DevBuf<uint2> cin, ent;
    DevBuf<ferhip_rtp_pkt> dp;
    DevBuf<ferhip_rtp_au> idx;
    if (src.reserve(pitch * n) || dst.reserve(std::max<size_t>(cap, 16)) || dl.reserve(n) || dh.reserve(3 * n) || dt.reserve(n) ||
        summ.reserve(n * nchmax) || cin.reserve(n * nchmax) || ent.reserve(n) || dp.reserve(std::max<size_t>(pkts_cap, 1)) || idx.reserve(n + 1))
        return FERHIP_E_HIP;
    CK(hipMemset(src, 0, pitch * n));
    if (maxlen) CK(hipMemcpy2D(src, pitch, payloads, stride, maxlen, n, hipMemcpyHostToDevice));
    CK(hipMemcpy(dl, lens, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(dh, hdr, sizeof(ferhip_rtp_hdr) * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(dt, nal_type, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    if (cap) CK(hipMemcpy(dst, out, cap, hipMemcpyHostToDevice));
    if (pkts_cap) CK(hipMemcpy(dp, pkts, sizeof(ferhip_rtp_pkt) * pkts_cap, hipMemcpyHostToDevice));
    FerRtpJob j;
    j.nal.src = src;
    j.nal.src_stride = pitch;
    j.nal.lens = dl;
    j.nal.hdr = nullptr;
    j.nal.types = dt;
    j.nal.ps = nullptr;
    j.nal.avcc = 0;
    j.nal.n = (int)n;
    j.nal.nchmax = nchmax;
    j.nal.summ = summ;
    j.nal.cin = cin;
    j.nal.ent = ent;
    j.nal.index = nullptr;
    j.nal.dst = nullptr;
    j.nal.cap = 0;
    j.ps = nullptr;
    j.hdr = dh;
    j.P = (uint32_t)max_packet;
    j.dst = dst;
    j.cap = cap;
    j.pkts = dp;
    j.pkts_cap = pkts_cap;
    j.index = idx;
    rtp_launch_plan(j, nullptr);
    rtp_launch_emit(j, nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    if (cap) CK(hipMemcpy(out, dst, cap, hipMemcpyDeviceToHost));
    if (pkts_cap) CK(hipMemcpy(pkts, dp, sizeof(ferhip_rtp_pkt) * pkts_cap, hipMemcpyDeviceToHost));
    CK(hipMemcpy(index, idx, sizeof(ferhip_rtp_au) * (n + 1), hipMemcpyDeviceToHost));
    return 0;  // the temporaries go with their owners
}

// ---- the way in: packets in device memory -> every stream's units behind 4-byte lengths, which fer_split_run takes
struct FerUnrtpJob {
    const uint8_t *base;
    const ferhip_rtp_pkt *pkts;  // sorted by stream
    uint32_t npk;
    int S;
    uint4 *rec, *piece;
    const uint32_t *first;       // [S + 1]
    const unsigned long long *sbase;  // [S] every stream's place in the staging buffer
    const int32_t *expect;       // [S]
    int32_t *res;                // [3][S] staged bytes, fault, expectation out
    uint8_t *stage;
};
#define UNRTP_BAD_HEADER 0u
#define UNRTP_SINGLE 1u
#define UNRTP_STAP 2u
#define UNRTP_FU 3u
#define UNRTP_BAD_PAYLOAD 4u

// One lane per packet: its header (steps 1 and 3 of the definition as far as one packet tells) -> x = kind | S << 8 | E << 9 |
// the unit's header byte << 16, y = where the payload begins in the packet, z = its bytes, w = seq.  Byte loads, inside the
// packet only.
__global__ __launch_bounds__(256) void k_unrtp_parse(FerUnrtpJob j)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= j.npk) return;
    const uint8_t *p = j.base + j.pkts[k].offset;
    const uint32_t L = j.pkts[k].bytes;
    uint4 r = make_uint4(UNRTP_BAD_HEADER, 0u, 0u, 0u);
    do {
        if (L < 12u || p[0] >> 6 != 2u) break;
        uint32_t hl = 12u + 4u * (p[0] & 15u);
        if (p[0] & 0x10u) {
            if (hl + 4u > L) break;
            hl += 4u + 4u * ((uint32_t)p[hl + 2u] << 8 | p[hl + 3u]);
            if (hl > L) break;
        }
        uint32_t pad = 0u;
        if (p[0] & 0x20u) {
            pad = p[L - 1u];
            if (pad < 1u) break;
        }
        if (hl + pad >= L) break;
        const uint32_t n = L - pad - hl, b0 = p[hl], t = b0 & 31u;
        r.y = hl;
        r.z = n;
        r.w = (uint32_t)p[2] << 8 | p[3];
        if (t >= 1u && t <= 23u)
            r.x = UNRTP_SINGLE;
        else if (t == 24u)
            r.x = UNRTP_STAP;
        else if (t == 28u && n >= 2u && (p[hl + 1u] & 0xC0u) != 0xC0u)
            r.x = UNRTP_FU | (p[hl + 1u] & 0x80u ? 0x100u : 0u) | (p[hl + 1u] & 0x40u ? 0x200u : 0u) | ((b0 & 0xE0u) | (p[hl + 1u] & 0x1Fu)) << 16;
        else
            r.x = UNRTP_BAD_PAYLOAD;
    } while (0);
    j.rec[k] = r;
}

__device__ __forceinline__ void unrtp_len32(uint8_t *w, uint32_t v) { w[0] = (uint8_t)(v >> 24), w[1] = (uint8_t)(v >> 16), w[2] = (uint8_t)(v >> 8), w[3] = (uint8_t)v; }

// One wavefront per stream, of which lane 0 walks the stream's records in order: the sequence check and the FU-A state are
// serial.  It writes the 4-byte lengths, the header byte of a fragmented unit and the (small) units of a STAP-A packet
// itself, and leaves one piece per packet for k_unrtp_gather: (source low, source high, bytes, place).  A stream's staging
// range holds at most 5/3 of its packets' bytes (a STAP-A entry of 2 + 1 bytes becomes 4 + 1), which the host reserved.
__global__ __launch_bounds__(64) void k_unrtp_walk(FerUnrtpJob j)
{
    const int s = blockIdx.x;
    if (threadIdx.x != 0) return;
    uint8_t *stage = j.stage + j.sbase[s];
    int32_t expect = j.expect[s], fault = 0;
    uint32_t w = 0u, lenpos = 0u, ulen = 0u;
    bool open = false;
    uint32_t k = j.first[s];
    const uint32_t end = j.first[s + 1];
    for (; k < end && !fault; k++) {
        const uint4 r = j.rec[k];
        const uint32_t kind = r.x & 255u;
        uint4 piece = make_uint4(0u, 0u, 0u, 0u);
        if (kind == UNRTP_BAD_HEADER)
            fault = 2;
        else if (expect >= 0 && (int32_t)r.w != expect)
            fault = 3;
        else {
            expect = (int32_t)((r.w + 1u) & 0xffffu);
            const unsigned long long src = j.pkts[k].offset + r.y;
            if ((open && kind != UNRTP_FU) || kind == UNRTP_BAD_PAYLOAD) {
                fault = 2;
            } else if (kind == UNRTP_SINGLE) {
                unrtp_len32(stage + w, r.z);
                piece = make_uint4((uint32_t)src, (uint32_t)(src >> 32), r.z, w + 4u);
                w += 4u + r.z;
            } else if (kind == UNRTP_STAP) {
                const uint8_t *p = j.base + src;
                uint32_t pos = 1u;
                if (pos == r.z) fault = 2;
                while (pos < r.z && !fault) {
                    if (r.z - pos < 2u) {
                        fault = 2;
                        break;
                    }
                    const uint32_t size = (uint32_t)p[pos] << 8 | p[pos + 1u];
                    pos += 2u;
                    if (size == 0u || size > r.z - pos) {
                        fault = 2;
                        break;
                    }
                    unrtp_len32(stage + w, size);
                    for (uint32_t i = 0; i < size; i++) stage[w + 4u + i] = p[pos + i];
                    w += 4u + size;
                    pos += size;
                }
            } else {
                const bool S = (r.x & 0x100u) != 0u, E = (r.x & 0x200u) != 0u;
                if (S == open) {  // S while one is open, or a fragment without S while none is
                    fault = 2;
                } else {
                    if (S) {
                        lenpos = w;
                        stage[w + 4u] = (uint8_t)(r.x >> 16);
                        w += 5u;
                        ulen = 1u;
                        open = true;
                    }
                    piece = make_uint4((uint32_t)(src + 2ull), (uint32_t)((src + 2ull) >> 32), r.z - 2u, w);
                    w += r.z - 2u;
                    ulen += r.z - 2u;
                    if (E) {
                        unrtp_len32(stage + lenpos, ulen);
                        open = false;
                    }
                }
            }
        }
        j.piece[k] = piece;
    }
    for (; k < end; k++) j.piece[k] = make_uint4(0u, 0u, 0u, 0u);
    if (open && !fault) fault = 4;
    if (open) w = lenpos;  // the unit that was not completed is no unit (its pieces land behind the range's end)
    j.res[s] = (int32_t)w;
    j.res[j.S + s] = fault;
    j.res[2 * j.S + s] = fault ? -1 : expect;
}

// grid (packet): the packet's piece, byte by byte (source and place have any alignment)
__global__ __launch_bounds__(256) void k_unrtp_gather(FerUnrtpJob j)
{
    const uint32_t k = blockIdx.x;
    const uint4 pc = j.piece[k];
    if (pc.z == 0u) return;
    const uint8_t *src = j.base + ((unsigned long long)pc.y << 32 | pc.x);
    uint8_t *dst = j.stage + j.sbase[j.pkts[k].stream] + pc.w;
    for (uint32_t i = threadIdx.x; i < pc.z; i += 256u) dst[i] = src[i];
}

int fer_unrtp_run(FerUnrtp &u, hipStream_t st, const uint8_t *d_base, const ferhip_rtp_pkt *pkts, size_t npk, const uint32_t *first, int S,
                  int32_t *expect, int32_t *fault)
{
    u.ptrs.assign(S, nullptr);
    u.lens.assign(S, 0);
    for (int s = 0; s < S; s++) fault[s] = 0;
    if (npk == 0) return 0;
    if (npk > 0xffffffffull) return FERHIP_E_ARG;
    // job words: first[S + 1], expectation[S], then the staging bases as 64-bit values (8-byte aligned)
    const size_t words = ((size_t)(2 * S + 1) + 1) & ~(size_t)1;
    if (u.d_pkts.reserve(npk, npk + npk / 4) || u.h_pkts.reserve(npk, npk + npk / 4) || u.d_rec.reserve(npk, npk + npk / 4) ||
        u.d_piece.reserve(npk, npk + npk / 4) || u.d_job.reserve(words + 2 * (size_t)S) || u.h_job.reserve(words + 2 * (size_t)S) ||
        u.d_res.reserve(3 * (size_t)S) || u.h_res.reserve(3 * (size_t)S))
        return FERHIP_E_HIP;
    memcpy(u.h_pkts, pkts, npk * sizeof(ferhip_rtp_pkt));
    uint32_t *hj = u.h_job;
    unsigned long long *hb = (unsigned long long *)(hj + words);
    unsigned long long total = 0;
    for (int s = 0; s < S; s++) {
        hj[s] = first[s];
        hj[S + 1 + s] = (uint32_t)expect[s];
        hb[s] = total;
        unsigned long long bytes = 0;
        for (uint32_t k = first[s]; k < first[s + 1]; k++) bytes += pkts[k].bytes;
        total += (bytes * 5 / 3 + 8 + 15) & ~15ull;
    }
    hj[S] = first[S];
    if (u.d_stage.reserve((size_t)total, (size_t)(total + total / 4))) return FERHIP_E_HIP;
    CK(hipMemcpyAsync(u.d_pkts, u.h_pkts, npk * sizeof(ferhip_rtp_pkt), hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(u.d_job, u.h_job, (words + 2 * (size_t)S) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    FerUnrtpJob j;
    j.base = d_base;
    j.pkts = u.d_pkts;
    j.npk = (uint32_t)npk;
    j.S = S;
    j.rec = u.d_rec;
    j.piece = u.d_piece;
    j.first = u.d_job;
    j.expect = (const int32_t *)(u.d_job.p + S + 1);
    j.sbase = (const unsigned long long *)(u.d_job.p + words);
    j.res = u.d_res;
    j.stage = u.d_stage;
    hipLaunchKernelGGL(k_unrtp_parse, dim3((unsigned)((npk + 255) / 256)), dim3(256), 0, st, j);
    hipLaunchKernelGGL(k_unrtp_walk, dim3(S), dim3(64), 0, st, j);
    hipLaunchKernelGGL(k_unrtp_gather, dim3((unsigned)npk), dim3(256), 0, st, j);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(u.h_res, u.d_res, 3 * (size_t)S * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    CK(hipStreamSynchronize(st));  // the pinned job words may be rewritten from here on, too
    for (int s = 0; s < S; s++) {
        u.lens[s] = (size_t)u.h_res[s];
        u.ptrs[s] = u.lens[s] ? u.d_stage.p + hb[s] : nullptr;
        fault[s] = u.h_res[S + s];
        expect[s] = u.h_res[2 * S + s];
    }
    return 0;
}

// rows sorted by stream (stable) and every stream's first row; false for a stream outside [0, S)
static bool rtp_sort(const ferhip_rtp_pkt *pkts, size_t npk, int S, std::vector<ferhip_rtp_pkt> &sorted, std::vector<uint32_t> &first)
{
    first.assign((size_t)S + 1, 0);
    for (size_t k = 0; k < npk; k++) {
        if (pkts[k].stream >= (uint32_t)S) return false;
        first[pkts[k].stream + 1]++;
    }
    for (int s = 0; s < S; s++) first[s + 1] += first[s];
    sorted.resize(npk);
    std::vector<uint32_t> at(first.begin(), first.end() - 1);
    for (size_t k = 0; k < npk; k++) sorted[at[pkts[k].stream]++] = pkts[k];
    return true;
}
int fer_rtp_sort(const ferhip_rtp_pkt *pkts, size_t npk, int S, std::vector<ferhip_rtp_pkt> &sorted, std::vector<uint32_t> &first)
{
    return rtp_sort(pkts, npk, S, sorted, first) ? 0 : FERHIP_E_ARG;
}

// known-answer surface of the way in: host packets through the same kernels and the splitter, on the null stream
extern "C" int ferhip_unrtp_blocks(const uint8_t *base, size_t base_bytes, const ferhip_rtp_pkt *pkts, size_t npkts, int nstreams, int misalign,
                                   const int32_t *seq_expect, uint8_t *out, size_t cap, ferhip_nal_unit *units, size_t units_cap,
                                   size_t *nunits, int32_t *fault, int32_t *seq_next)
{
    if (nunits) *nunits = 0;
    if (!nunits || !fault || !seq_next || !seq_expect || nstreams <= 0 || nstreams > 65535 || misalign < 0 || misalign > 15 || (!out && cap) ||
        (!units && units_cap) || (npkts && (!base || !pkts)))
        return FERHIP_E_ARG;
    for (size_t k = 0; k < npkts; k++)
        if (pkts[k].offset > base_bytes || pkts[k].bytes > base_bytes - pkts[k].offset) return FERHIP_E_ARG;
    std::vector<ferhip_rtp_pkt> sorted;
    std::vector<uint32_t> first;
    if (!rtp_sort(pkts, npkts, nstreams, sorted, first)) return FERHIP_E_ARG;
    DevBuf<uint8_t> dbase, dst;
    FerUnrtp u;
    FerSplit sp;
    if (dbase.reserve((size_t)misalign + std::max<size_t>(base_bytes, 1)) || dst.reserve(std::max<size_t>(cap, 16))) return FERHIP_E_HIP;
    if (base_bytes) CK(hipMemcpy(dbase + misalign, base, base_bytes, hipMemcpyHostToDevice));
    if (cap) CK(hipMemcpy(dst, out, cap, hipMemcpyHostToDevice));
    for (int s = 0; s < nstreams; s++) seq_next[s] = seq_expect[s];
    if (int rc = fer_unrtp_run(u, nullptr, dbase + misalign, sorted.data(), npkts, first.data(), nstreams, seq_next, fault)) return rc;
    size_t staged = 0;
    for (size_t n : u.lens) staged += n;
    if (!staged) return 0;  // no unit at all: nothing for the splitter
    if (int rc = fer_split_run(sp, nullptr, u.ptrs.data(), u.lens.data(), nstreams, dst, cap, 4)) return rc;
    if (cap) CK(hipMemcpy(out, dst, cap, hipMemcpyDeviceToHost));
    size_t k = 0;
    fer_split_each_unit(sp, [&](size_t, const ferhip_nal_unit &un) {
        if (k < units_cap) units[k] = un;
        k++;
        return 0;
    });
    *nunits = k;
    return k > units_cap || (size_t)sp.head()->bytes > cap ? FERHIP_E_ARG : 0;
}

static size_t b64(const uint8_t *p, size_t n, char *out)
{
    static const char tab[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
    char *w = out;
    for (size_t i = 0; i < n; i += 3) {
        const uint32_t v = (uint32_t)p[i] << 16 | (i + 1 < n ? (uint32_t)p[i + 1] << 8 : 0u) | (i + 2 < n ? (uint32_t)p[i + 2] : 0u);
        *w++ = tab[v >> 18];
        *w++ = tab[(v >> 12) & 63];
        *w++ = i + 1 < n ? tab[(v >> 6) & 63] : '=';
        *w++ = i + 2 < n ? tab[v & 63] : '=';
    }
    return (size_t)(w - out);
}

// the format parameters of stream s for SDP (RFC 6184 section 8.1): one SPS and the stream's own PPS
extern "C" size_t ferhip_write_sdp_fmtp(ferhip_ctx *c, int s, char *out, size_t cap)
{
    if (!c || !out || s < 0 || s >= c->d.S) return 0;
    uint8_t rbsp[64], sps[2 * (5 + 96)], pps[2 * (5 + 96)];
    size_t n = ferhip_write_sps(c, rbsp, sizeof rbsp);
    if (n < 3) return 0;
    char text[96 + 2 * 4 * ((2 * (5 + 96) + 2) / 3)];  // 67 characters, two units in base64, a comma
    size_t m = (size_t)snprintf(text, sizeof text, "profile-level-id=%02x%02x%02x;packetization-mode=1;sprop-parameter-sets=", rbsp[0], rbsp[1],
                                rbsp[2]);
    const size_t ns = ferhip_write_nal(1, 7, rbsp, n, sps) - 4;  // the unit behind its start code
    n = ferhip_write_pps_stream(c, s, rbsp, sizeof rbsp);
    if (n == 0) return 0;
    const size_t np = ferhip_write_nal(1, 8, rbsp, n, pps) - 4;
    m += b64(sps + 4, ns, text + m);
    text[m++] = ',';
    m += b64(pps + 4, np, text + m);
    if (m + 1 > cap) return 0;
    memcpy(out, text, m);
    out[m] = 0;
    return m;
}
