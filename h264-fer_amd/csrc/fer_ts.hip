// fer_ts.hip -- the coded pictures as an MPEG-2 transport stream (ISO/IEC 13818-1) on the device (ferhip_pack_ts,
// ferhip_fetch_ts, ferhip_ts_blocks; the definition stands in include/ferhip.h): every access unit -- a delimiter, then the
// entry ferhip_pack_nal writes -- is one PES packet, cut into 188-byte packets, with a PCR in its first packet and, where
// asked for, a PAT and a PMT packet in front of an I picture; and the way in (ferhip_decs_decode_ts, ferhip_unts_blocks).
//
// The bytes that are cut into packets are the escaped ones, so the emulation prevention comes first, and it is fer_nalpack.hip's:
//   k_nal_count, k_nal_plan   run as they are (fer_launch_nal_count): every 4096-byte chunk's incoming counter and the 03
//                bytes in front of it, and the entry's size.
//   k_ts_index   one wavefront: a lane takes a stream, derives the PES packet's length L and its packet count from the
//                entry's size, and the exclusive sum over the streams gives the index.
//   k_ts_emit    grid (chunk, stream): the scan of k_nal_emit gives every lane its position in the escaped payload, hence its
//                PES byte x; from x follow its packet and its offset in that packet (TsPlan::place).  A stream's output is one
//                contiguous range, so the chunk builds its span in LDS in output coordinates: its PES bytes, the 4-byte
//                headers of the packets whose first payload byte it holds and, for the first and the last packet, the
//                adaptation field with its stuffing.  The span goes out with store_span.  Chunk 0 also places the PES header,
//                the delimiter, the parameter sets from the table, the five bytes in front of the payload and the two PSI
//                packets from their table, with psi_cc patched in.
// No workgroup waits for another one: the phases are separate launches on one stream.
// The way in: k_unts_parse (a lane per packet), k_unts_walk (a wavefront per stream), k_unts_gather, then fer_split_run on
// the staged elementary-stream bytes as Annex-B.
#include "fer_nal.h"
#include "fer_nalsplit.h"
#include <string.h>
#include <algorithm>

#define TS_PKT 188u
#define TS_PSI_ROW 376  // a PAT and a PMT packet

struct FerTsJob {
    FerNalJob nal;             // index / dst unused; ps = the table with FERHIP_AU_PARAM_SETS: ent[] then counts them
    const ferhip_ts_hdr *hdr;  // [n] device
    const uint8_t *psi;        // [n][TS_PSI_ROW] or null: the two PSI packets in front of an I picture
    uint8_t *dst;
    unsigned long long cap;
    ferhip_ts_au *index;       // [n + 1] device
};

// The packets of one stream's access unit, from the size of its entry.  PES byte x lies in packet 0 while x < 176 (a single
// packet holds all L <= 176 of them, right-aligned), else in packet 1 + (x - 176) / 184; the last packet is right-aligned.
struct TsPlan {
    uint32_t L;      // PES packet: 14 header bytes, 6 of the delimiter, the entry
    uint32_t n;      // packets that carry it
    uint32_t clast;  // PES bytes in the last of them
    uint32_t pslen;  // the parameter sets in front of the slice unit
    uint32_t psi;    // bytes of PSI packets in front: 0 or TS_PSI_ROW
    // where the payload begins in packet k
    __device__ __forceinline__ uint32_t paystart(uint32_t k) const { return k == n - 1u ? TS_PKT - clast : (k == 0u ? 12u : 4u); }
    // PES byte x -> its place counted from the stream's first PES-carrying packet; k = its packet, room = the PES bytes of
    // that packet from x on
    __device__ __forceinline__ uint32_t place(uint32_t x, uint32_t &k, uint32_t &room) const
    {
        uint32_t w = x, c = L;
        k = 0u;
        if (n > 1u) {
            c = 176u;
            if (x >= 176u) {
                k = 1u + (x - 176u) / 184u;
                w = x - 176u - (k - 1u) * 184u;
                c = k == n - 1u ? clast : 184u;
            }
        }
        room = c - w;
        return k * TS_PKT + paystart(k) + w;
    }
};

// ent = k_nal_plan's (entry size, type) of a stream that is there
__device__ __forceinline__ TsPlan ts_plan(const FerTsJob &j, int s, const uint2 &ent)
{
    TsPlan p;
    const bool idr = ent.y == (uint32_t)FERHIP_NAL_IDR;
    p.pslen = (j.nal.ps && idr) ? j.nal.ps[(size_t)s * FER_NAL_PS_ROW + FER_NAL_PS_ROW - 1] : 0u;
    p.L = 20u + ent.x;
    p.n = p.L <= 176u ? 1u : 1u + (p.L - 176u + 183u) / 184u;
    p.clast = p.n == 1u ? p.L : p.L - 176u - (p.n - 2u) * 184u;
    p.psi = (j.psi && idr) ? (uint32_t)TS_PSI_ROW : 0u;
    return p;
}

__global__ __launch_bounds__(64) void k_ts_index(FerTsJob j)
{
    const int lane = threadIdx.x, n = j.nal.n;
    unsigned long long run = 0, prun = 0;
    uint32_t written = 0;
    for (int s0 = 0; s0 < n; s0 += 64) {
        const int s = s0 + lane;
        const uint2 e = s < n ? j.nal.ent[s] : make_uint2(0u, 0u);
        unsigned long long np = 0;
        if (e.x) {
            const TsPlan p = ts_plan(j, s, e);
            np = p.n + p.psi / TS_PKT;
        }
        const unsigned long long bytes = np * TS_PKT, r = (bytes + 15ull) & ~15ull;
        const unsigned long long incl = wave_scan(r, lane, ScanAdd()), pincl = wave_scan(np, lane, ScanAdd());
        const unsigned long long off = run + incl - r;
        if (s < n) {
            ferhip_ts_au a;
            a.offset = e.x ? off : 0ull;
            a.bytes = (uint32_t)bytes;
            a.nal_type = e.x ? (int32_t)e.y : 0;
            a.npkts = (uint32_t)np;
            a.reserved = 0u;
            j.index[s] = a;
        }
        written += (uint32_t)__popcll(__ballot(e.x != 0u && off + bytes <= j.cap));
        run += __shfl(incl, 63);
        prun += __shfl(pincl, 63);
    }
    if (lane == 0) {
        ferhip_ts_au a;
        a.offset = run;
        a.bytes = written;
        a.nal_type = 0;
        a.npkts = (uint32_t)prun;
        a.reserved = 0u;
        j.index[n] = a;
    }
}

// LDS image of one chunk's output.  A chunk holds at most NAL_CHUNK + NAL_CHUNK / 2 + 1 = 6145 escaped bytes, and chunk 0
// has 25 + FER_NAL_PS_ROW PES bytes in front of them: TS_NB = 6234 PES bytes at most.  A packet carries at most 184 of them,
// and they begin anywhere in a packet, so they touch at most 1 + (TS_NB - 1 + 183) / 184 = 35 packets (packet 0 carries 176
// only, but a chunk that holds any byte of packet 0 is chunk 0 and begins with it).  The chunk's span lies within those
// packets, of 188 bytes each, behind the PSI packets (chunk 0) and up to 15 bytes of misalignment: 15 + 376 + 35 * 188 = 6971.
#define TS_NB (NAL_CHUNK + NAL_CHUNK / 2 + 1 + 25 + FER_NAL_PS_ROW)
#define TS_IMG ((15 + TS_PSI_ROW + 188 * (1 + (TS_NB - 1 + 183) / 184) + 15) & ~15)
static_assert(TS_IMG == 6976 && TS_IMG + 64 <= 65536, "the chunk's span and the scan's totals fit the LDS of a workgroup");

// byte b < paystart(k) of packet k: the 4-byte header, then the adaptation field -- with the PCR in packet 0 -- and stuffing
__device__ __forceinline__ uint8_t ts_hdr_byte(const TsPlan &p, uint32_t k, uint32_t b, const ferhip_ts_hdr &h, bool idr)
{
    const uint32_t ps = p.paystart(k);
    switch (b) {
    case 0: return 0x47;
    case 1: return (uint8_t)((k == 0u ? 0x40u : 0u) | (uint32_t)h.pid >> 8);
    case 2: return (uint8_t)h.pid;
    case 3: return (uint8_t)((ps > 4u ? 0x30u : 0x10u) | ((h.cc + k) & 15u));
    case 4: return (uint8_t)(ps - 5u);
    default: break;
    }
    if (k != 0u) return b == 5u ? 0x00 : 0xFF;
    switch (b) {
    case 5: return (uint8_t)(0x10u | (idr ? 0x40u : 0u));
    case 6: return (uint8_t)(h.pcr >> 25);
    case 7: return (uint8_t)(h.pcr >> 17);
    case 8: return (uint8_t)(h.pcr >> 9);
    case 9: return (uint8_t)(h.pcr >> 1);
    case 10: return (uint8_t)(((uint32_t)(h.pcr & 1ull) << 7) | 0x7Eu);
    case 11: return 0x00;
    default: return 0xFF;
    }
}

// PES byte x < 25 + pslen of a stream: the PES header, the delimiter, the parameter sets, the start code and the header byte
__device__ __forceinline__ uint8_t ts_head_byte(const TsPlan &p, uint32_t x, const ferhip_ts_hdr &h, uint32_t type, const uint8_t *row)
{
    if (x < 14u) {
        switch (x) {
        case 2: return 0x01;
        case 3: return 0xE0;
        case 6: return 0x84;
        case 7: return 0x80;
        case 8: return 0x05;
        case 9: return (uint8_t)(0x21u | ((uint32_t)(h.pts >> 29) & 0x0Eu));
        case 10: return (uint8_t)(h.pts >> 22);
        case 11: return (uint8_t)(0x01u | ((uint32_t)(h.pts >> 14) & 0xFEu));
        case 12: return (uint8_t)(h.pts >> 7);
        case 13: return (uint8_t)(0x01u | ((uint32_t)(h.pts << 1) & 0xFEu));
        default: return 0x00;
        }
    }
    if (x < 20u) return x == 17u ? 0x01 : x == 18u ? 0x09 : x == 19u ? (type == (uint32_t)FERHIP_NAL_IDR ? 0x10 : 0x30) : 0x00;
    if (x < 20u + p.pslen) return row[x - 20u];
    const uint32_t k = x - 20u - p.pslen;
    return k < 3u ? 0x00 : k == 3u ? 0x01 : (uint8_t)(1u << 5 | (type & 31u));
}

__global__ __launch_bounds__(NAL_THREADS) void k_ts_emit(FerTsJob j)
{
    const int s = blockIdx.y;
    const ferhip_ts_au au = j.index[s];
    if (au.npkts == 0u || au.offset + au.bytes > j.cap) return;  // no picture, or packets that do not end within cap
    const uint2 ent = j.nal.ent[s];
    const TsPlan p = ts_plan(j, s, ent);
    const ferhip_ts_hdr h = j.hdr[s];
    const bool idr = ent.y == (uint32_t)FERHIP_NAL_IDR;
    const uint32_t head = 25u + p.pslen;  // PES bytes in front of the escaped payload
    const uint32_t len = nal_len(j.nal, s);
    const uint32_t nch = max((len + NAL_CHUNK - 1) / NAL_CHUNK, 1u);  // an empty payload still has its head
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __shared__ uint4 wtot[NAL_THREADS / 64];
    __shared__ __attribute__((aligned(16))) uint8_t img[TS_IMG];

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
        // the chunk's PES bytes [xa, xb): its escaped bytes [e0, e1) of the payload, and in chunk 0 the head
        const uint32_t nin = len > chunk * NAL_CHUNK ? min((uint32_t)NAL_CHUNK, len - chunk * NAL_CHUNK) : 0u;
        const uint32_t e0 = chunk * NAL_CHUNK + cin.y, e1 = e0 + nin + nal_cnt(tot, cin.x);
        const uint32_t xa = chunk ? head + e0 : 0u, xb = head + e1;
        uint32_t ka, kl, room;
        const uint32_t qa = p.place(xa, ka, room), ql = p.place(xb - 1u, kl, room);
        // a packet is begun by the chunk that holds its first payload byte: packets [kb, ke)
        const bool begins = qa == ka * TS_PKT + p.paystart(ka);
        const uint32_t kb = begins ? ka : ka + 1u, ke = kl + 1u;
        // span [rstart, rend) in bytes from the stream's offset, staged in img from rbase = rstart rounded down to 16
        const uint32_t rstart = chunk ? p.psi + (begins ? ka * TS_PKT : qa) : 0u, rend = p.psi + ql + 1u;
        const uint32_t rbase = rstart & ~15u, org = p.psi - rbase;  // img[org + place] (mod 2^32: rbase <= psi + place)
        if (!chunk) {
            for (uint32_t t = (uint32_t)tid; t < p.psi; t += NAL_THREADS) {
                const uint8_t b = j.psi[(size_t)s * TS_PSI_ROW + t];
                img[t] = (t == 3u || t == TS_PKT + 3u) ? (uint8_t)(0x10u | (h.psi_cc & 15u)) : b;
            }
            if ((uint32_t)tid < head)
                img[org + p.paystart(0u) + (uint32_t)tid] = ts_head_byte(p, (uint32_t)tid, h, ent.y, p.pslen ? j.nal.ps + (size_t)s * FER_NAL_PS_ROW : nullptr);
        }
        for (uint32_t t = (uint32_t)tid; t < (ke - kb) * 4u; t += NAL_THREADS) {
            const uint32_t k = kb + (t >> 2), b = t & 3u;
            img[org + k * TS_PKT + b] = ts_hdr_byte(p, k, b, h, idr);
        }
        // the adaptation fields: packet 0's, and the last packet's where it is another one
        if (kb == 0u && 4u + (uint32_t)tid < p.paystart(0u)) img[org + 4u + (uint32_t)tid] = ts_hdr_byte(p, 0u, 4u + (uint32_t)tid, h, idr);
        if (p.n > 1u && kb <= p.n - 1u && p.n - 1u < ke && 4u + (uint32_t)tid < p.paystart(p.n - 1u))
            img[org + (p.n - 1u) * TS_PKT + 4u + (uint32_t)tid] = ts_hdr_byte(p, p.n - 1u, 4u + (uint32_t)tid, h, idr);
        if (nvalid) {
            uint32_t z = nal_out(excl, cin.x);
            uint32_t k;
            uint32_t q = org + p.place(head + e0 + (uint32_t)tid * 16u + nal_cnt(excl, cin.x), k, room);
#define TS_PUT(x)                                       \
    {                                                   \
        img[q++] = (uint8_t)(x);                        \
        if (--room == 0u) {                             \
            k++;                                        \
            q += p.paystart(k);                         \
            room = k == p.n - 1u ? p.clast : 184u;      \
        }                                               \
    }
#define NAL_DWORD(wd, kk)                                  \
    _Pragma("unroll") for (int qq = 0; qq < 4; qq++)       \
    {                                                      \
        if (4 * (kk) + qq < nvalid) {                      \
            const uint32_t b = ((wd) >> (8 * qq)) & 0xffu; \
            if (nal_step(b, z)) TS_PUT(3)                  \
            TS_PUT(b)                                      \
        }                                                  \
    }
            NAL_DWORD(v.x, 0)
            NAL_DWORD(v.y, 1)
            NAL_DWORD(v.z, 2)
            NAL_DWORD(v.w, 3)
#undef NAL_DWORD
#undef TS_PUT
        }
        __syncthreads();
        // the stream's packets end within cap (above): nothing to cut
        store_span<NAL_THREADS>(j.dst + au.offset + rbase, img, rstart - rbase, rend - rbase);
        __syncthreads();
    }
}

static void ts_launch_plan(const FerTsJob &j, hipStream_t st)
{
    fer_launch_nal_count(j.nal, st);
    hipLaunchKernelGGL(k_ts_index, dim3(1), dim3(64), 0, st, j);
}

static void ts_launch_emit(const FerTsJob &j, hipStream_t st)
{
    hipLaunchKernelGGL(k_ts_emit, dim3(nal_grid_x(j.nal), j.nal.n), dim3(NAL_THREADS), 0, st, j);
}

static bool ts_pid_ok(unsigned pid) { return pid >= 0x0010u && pid <= 0x1FFEu; }

static bool ts_args_ok(int flags, const ferhip_ts_hdr *hdr, size_t n)
{
    if ((flags & ~(FERHIP_AU_PARAM_SETS | FERHIP_TS_PSI)) || !hdr) return false;
    for (size_t s = 0; s < n; s++) {
        const ferhip_ts_hdr &h = hdr[s];
        if (h.pts >> 33 || h.pcr >> 33 || !ts_pid_ok(h.pid) || !ts_pid_ok(h.pmt_pid) || h.pid == h.pmt_pid || h.cc > 15 || h.psi_cc > 15 ||
            h.reserved != 0)
            return false;
    }
    return true;
}

// CRC-32/MPEG-2 over a section from its table_id
static uint32_t ts_crc(const uint8_t *p, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) {
        c ^= (uint32_t)p[i] << 24;
        for (int b = 0; b < 8; b++) c = (c & 0x80000000u) ? (c << 1) ^ 0x04C11DB7u : c << 1;
    }
    return c;
}

// one PSI packet: header, pointer_field 0, the section with its CRC, FF to the end
static void ts_psi_packet(uint8_t *out, unsigned pid, int cc, const uint8_t *section, size_t n)
{
    memset(out, 0xFF, TS_PKT);
    out[0] = 0x47;
    out[1] = (uint8_t)(0x40u | pid >> 8);
    out[2] = (uint8_t)pid;
    out[3] = (uint8_t)(0x10 | (cc & 15));
    out[4] = 0x00;
    memcpy(out + 5, section, n);
    const uint32_t c = ts_crc(section, n);
    out[5 + n] = (uint8_t)(c >> 24), out[6 + n] = (uint8_t)(c >> 16), out[7 + n] = (uint8_t)(c >> 8), out[8 + n] = (uint8_t)c;
}

extern "C" size_t ferhip_write_ts_psi(int pid, int pmt_pid, int psi_cc, uint8_t *out, size_t cap)
{
    if (!out || cap < TS_PSI_ROW || pid < 0 || pmt_pid < 0 || !ts_pid_ok((unsigned)pid) || !ts_pid_ok((unsigned)pmt_pid) || pid == pmt_pid ||
        psi_cc < 0 || psi_cc > 15)
        return 0;
    const uint8_t hi = (uint8_t)(0xE0 | pid >> 8), lo = (uint8_t)pid;
    const uint8_t pat[12] = {0x00, 0xB0, 0x0D, 0x00, 0x01, 0xC1, 0x00, 0x00, 0x00, 0x01, (uint8_t)(0xE0 | pmt_pid >> 8), (uint8_t)pmt_pid};
    const uint8_t pmt[17] = {0x02, 0xB0, 0x12, 0x00, 0x01, 0xC1, 0x00, 0x00, hi, lo, 0xF0, 0x00, 0x1B, hi, lo, 0xF0, 0x00};
    ts_psi_packet(out, 0u, psi_cc, pat, sizeof pat);
    ts_psi_packet(out + TS_PKT, (unsigned)pmt_pid, psi_cc, pmt, sizeof pmt);
    return TS_PSI_ROW;
}

// FERHIP_TS_PSI: the two PSI packets of every stream in the device table; a row is built and sent again only when the
// stream's (pid, pmt_pid) differ from what the table holds
static int ts_psi_refresh(ferhip_ctx *c, const ferhip_ts_hdr *hdr)
{
    const int S = c->d.S;
    if (c->ts_psi_ids.empty()) {
        if (dalloc(c, &c->d_ts_psi, (size_t)S * TS_PSI_ROW) || hipDeviceSynchronize() != hipSuccess || c->ts_psi_ring.create((size_t)S * TS_PSI_ROW)) {
            (void)hipGetLastError();
            return FERHIP_E_HIP;
        }
        c->ts_psi_ids.assign(S, 0u);  // no valid pair is 0
    }
    uint8_t *slot = nullptr;
    for (int s = 0; s < S; s++) {
        const uint32_t id = (uint32_t)hdr[s].pid << 16 | hdr[s].pmt_pid;
        if (c->ts_psi_ids[s] == id) continue;
        if (!slot && !(slot = (uint8_t *)c->ts_psi_ring.next())) return FERHIP_E_HIP;
        ferhip_write_ts_psi(hdr[s].pid, hdr[s].pmt_pid, 0, slot + (size_t)s * TS_PSI_ROW, TS_PSI_ROW);
        CK(hipMemcpyAsync(c->d_ts_psi + (size_t)s * TS_PSI_ROW, slot + (size_t)s * TS_PSI_ROW, TS_PSI_ROW, hipMemcpyHostToDevice, c->st));
        c->ts_psi_ids[s] = id;
    }
    return slot ? c->ts_psi_ring.sent(c->st) : 0;
}

// ---- host side: an encoder context's buffers, allocated on first use; hdr[] goes through the next slot of a pinned ring
static int ts_prepare(ferhip_ctx *c, int flags, const ferhip_ts_hdr *hdr, FerTsJob &j)
{
    static_assert(sizeof(ferhip_ts_hdr) == 24 && sizeof(ferhip_ts_au) == 24 && sizeof(ferhip_ts_run) == 16, "ABI");
    int rc = fer_nal_prepare(c, flags & FERHIP_AU_PARAM_SETS, j.nal);
    if (rc) return rc;
    const int S = c->d.S;
    if (!c->ts_ready) {  // dalloc, halloc and the ring keep what exists: a call after a failed one allocates what is missing
        if (dalloc(c, &c->ts_index, (size_t)S + 1) || halloc(c, &c->h_ts_index, (size_t)S + 1) || dalloc(c, &c->d_ts_hdr, (size_t)S) ||
            hipDeviceSynchronize() != hipSuccess ||  // dalloc clears on the null stream
            c->ts_ring.create((size_t)S * sizeof(ferhip_ts_hdr))) {
            (void)hipGetLastError();
            fprintf(stderr, "ferhip: could not allocate the TS buffers\n");
            return FERHIP_E_HIP;
        }
        c->ts_ready = true;
    }
    if ((flags & FERHIP_TS_PSI) && (rc = ts_psi_refresh(c, hdr))) return rc;
    void *slot = c->ts_ring.next();
    if (!slot) return FERHIP_E_HIP;
    memcpy(slot, hdr, (size_t)S * sizeof(ferhip_ts_hdr));
    CK(hipMemcpyAsync(c->d_ts_hdr, slot, (size_t)S * sizeof(ferhip_ts_hdr), hipMemcpyHostToDevice, c->st));
    if ((rc = c->ts_ring.sent(c->st))) return rc;
    j.hdr = c->d_ts_hdr;
    j.psi = (flags & FERHIP_TS_PSI) ? c->d_ts_psi : nullptr;
    j.dst = nullptr;
    j.cap = 0;
    j.index = c->ts_index;
    return 0;
}

extern "C" int ferhip_pack_ts(ferhip_ctx *c, int flags, const ferhip_ts_hdr *hdr, void *d_dst, size_t cap, ferhip_ts_au *d_index)
{
    if (!c || !d_index || !ts_args_ok(flags, hdr, (size_t)c->d.S) || ((uintptr_t)d_dst & 15) || ((uintptr_t)d_index & 7) || (!d_dst && cap))
        return FERHIP_E_ARG;
    FerTsJob j;
    int rc = ts_prepare(c, flags, hdr, j);
    if (rc) return rc;
    j.index = d_index;
    j.dst = (uint8_t *)d_dst;
    j.cap = cap;
    ts_launch_plan(j, c->st);
    ts_launch_emit(j, c->st);
    CK(hipGetLastError());
    return 0;
}

extern "C" int ferhip_fetch_ts(ferhip_ctx *c, int flags, const ferhip_ts_hdr *hdr, void *h_dst, size_t cap, ferhip_ts_au *h_index)
{
    if (!c || !h_index || !ts_args_ok(flags, hdr, (size_t)c->d.S) || (!h_dst && cap)) return FERHIP_E_ARG;
    FerTsJob j;
    int rc = ts_prepare(c, flags, hdr, j);
    if (rc) return rc;
    const int S = c->d.S;
    j.cap = cap;
    ts_launch_plan(j, c->st);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(c->h_ts_index, c->ts_index, sizeof(ferhip_ts_au) * (S + 1), hipMemcpyDeviceToHost, c->st));
    CK(hipStreamSynchronize(c->st));
    memcpy(h_index, c->h_ts_index, sizeof(ferhip_ts_au) * (S + 1));
    const size_t total = (size_t)c->h_ts_index[S].offset;
    if (total > cap) return FERHIP_E_ARG;
    if (total == 0) return 0;
    if (c->ts_buf.cap < total) {
        const size_t want = (total + total / 4 + 65535) & ~(size_t)65535;
        if (c->ts_buf.reserve(total, want)) return FERHIP_E_HIP;
        CK(hipMemsetAsync(c->ts_buf, 0, want, c->st));  // the bytes between streams are copied out too
    }
    j.dst = c->ts_buf;
    j.cap = total;
    ts_launch_emit(j, c->st);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(h_dst, c->ts_buf, total, hipMemcpyDeviceToHost, c->st));
    CK(hipStreamSynchronize(c->st));
    return 0;
}

// known-answer surface: host payloads through the same kernels, on the null stream with buffers of its own
extern "C" int ferhip_ts_blocks(const uint8_t *payloads, size_t stride, const uint32_t *lens, const int32_t *nal_type, size_t n,
                                const ferhip_ts_hdr *hdr, uint8_t *out, size_t cap, ferhip_ts_au *index)
{
    if (!lens || !nal_type || !index || n == 0 || n > 65535 || !ts_args_ok(0, hdr, n) || (!out && cap)) return FERHIP_E_ARG;
    uint32_t maxlen = 0;
    for (size_t i = 0; i < n; i++) {
        if (lens[i] > stride || lens[i] > (1u << 30) || (lens[i] && !payloads)) return FERHIP_E_ARG;
        maxlen = std::max(maxlen, lens[i]);
    }
    const size_t pitch = std::max<size_t>(((size_t)maxlen + 15) & ~(size_t)15, 16);
    const int nchmax = (int)std::max<size_t>(((size_t)maxlen + 4095) / 4096, 1);
    DevBuf<uint8_t> src, dst;
    DevBuf<uint32_t> dl;
    DevBuf<ferhip_ts_hdr> dh;
    DevBuf<int32_t> dt;
    DevBuf<uint4> summ;
    DevBuf<uint2> cin, ent;
    DevBuf<ferhip_ts_au> idx;
    if (src.reserve(pitch * n) || dst.reserve(std::max<size_t>(cap, 16)) || dl.reserve(n) || dh.reserve(n) || dt.reserve(n) ||
        summ.reserve(n * nchmax) || cin.reserve(n * nchmax) || ent.reserve(n) || idx.reserve(n + 1))
        return FERHIP_E_HIP;
    CK(hipMemset(src, 0, pitch * n));
    if (maxlen) CK(hipMemcpy2D(src, pitch, payloads, stride, maxlen, n, hipMemcpyHostToDevice));
    CK(hipMemcpy(dl, lens, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(dh, hdr, sizeof(ferhip_ts_hdr) * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(dt, nal_type, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    if (cap) CK(hipMemcpy(dst, out, cap, hipMemcpyHostToDevice));
    FerTsJob j;
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
    j.hdr = dh;
    j.psi = nullptr;
    j.dst = dst;
    j.cap = cap;
    j.index = idx;
    ts_launch_plan(j, nullptr);
    ts_launch_emit(j, nullptr);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    if (cap) CK(hipMemcpy(out, dst, cap, hipMemcpyDeviceToHost));
    CK(hipMemcpy(index, idx, sizeof(ferhip_ts_au) * (n + 1), hipMemcpyDeviceToHost));
    return 0;  // the temporaries go with their owners
}

// ---- the way in: packets in device memory -> every stream's elementary-stream bytes, one Annex-B range for fer_split_run
struct FerUntsJob {
    const uint8_t *base;
    const ferhip_ts_run *runs;   // sorted by stream
    const uint32_t *pfirst;      // [nruns + 1] every run's first packet
    uint32_t nruns, npk;
    int S;
    uint4 *rec, *piece;
    const uint32_t *sfirst;      // [S + 1] every stream's first packet
    const uint32_t *pids;        // [S]
    const int32_t *expect;       // [S]
    const unsigned long long *sbase;  // [S] every stream's place in the staging buffer
    int32_t *res;                // [3][S] staged bytes, fault, expectation out
    uint8_t *stage;
};
#define UNTS_BAD 0u      // rules 1, 3, 4: malformed before the counter is looked at
#define UNTS_SKIP 1u     // another PID, or no payload
#define UNTS_PAY 2u
#define UNTS_BAD_PES 3u  // rule 6: malformed behind the counter check

// One lane per packet, rules 1 to 4 and 6 -> x = kind | PUSI << 4 | counter << 8 | (where its elementary-stream bytes begin
// in the packet) << 16, y = how many they are, z and w = the packet's offset from base.  Byte loads, inside the packet only.
__global__ __launch_bounds__(256) void k_unts_parse(FerUntsJob j)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= j.npk) return;
    uint32_t lo = 0u, hi = j.nruns;  // the last run r with pfirst[r] <= k: the one that is not empty
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (j.pfirst[mid] <= k)
            lo = mid;
        else
            hi = mid;
    }
    const unsigned long long off = j.runs[lo].offset + (unsigned long long)(k - j.pfirst[lo]) * TS_PKT;
    const uint8_t *p = j.base + off;
    uint4 r = make_uint4(UNTS_BAD, 0u, (uint32_t)off, (uint32_t)(off >> 32));
    do {
        if (p[0] != 0x47u || (p[1] & 0x80u)) break;
        if ((((uint32_t)p[1] & 0x1Fu) << 8 | p[2]) != j.pids[j.runs[lo].stream]) {
            r.x = UNTS_SKIP;
            break;
        }
        const uint32_t b3 = p[3], afc = (b3 >> 4) & 3u;
        if (b3 >> 6 || afc == 0u) break;
        if (afc == 2u) {
            r.x = UNTS_SKIP;
            break;
        }
        uint32_t at = 4u;
        if (afc == 3u) {
            if (p[4] > 183u) break;
            at = 5u + p[4];
        }
        const uint32_t pusi = (p[1] >> 6) & 1u;
        r.x = UNTS_BAD_PES | pusi << 4 | (b3 & 15u) << 8;
        if (pusi) {
            const uint32_t n = TS_PKT - at;
            if (n < 9u || p[at] != 0u || p[at + 1u] != 0u || p[at + 2u] != 1u || (p[at + 3u] & 0xF0u) != 0xE0u || (p[at + 6u] & 0xC0u) != 0x80u ||
                n < 9u + p[at + 8u])
                break;
            at += 9u + p[at + 8u];
        }
        r.x = UNTS_PAY | pusi << 4 | (b3 & 15u) << 8 | at << 16;
        r.y = TS_PKT - at;
    } while (0);
    j.rec[k] = r;
}

// One wavefront per stream walks its packets in order, 64 to a step.  Within a step the ballot of the payload packets gives
// every one of them its predecessor's counter (the running expectation for the first), the ballot of the packets that begin
// a PES packet tells whether one is open in front of a lane, and the first lane with a fault ends the walk.  The packets in
// front of it get their place in the staging range by a wave scan over their elementary-stream bytes; the PES packet that is
// open at a fault is dropped by setting the range's end back to where it began (its pieces land behind the end).
__global__ __launch_bounds__(64) void k_unts_walk(FerUntsJob j)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    const unsigned long long lt = (1ull << lane) - 1ull;
    int32_t expect = j.expect[s], fault = 0;
    uint32_t w = 0u, pes_w = 0u;
    bool open = false;
    const uint32_t end = j.sfirst[s + 1];
    for (uint32_t k0 = j.sfirst[s]; k0 < end; k0 += 64u) {
        const uint32_t k = k0 + (uint32_t)lane;
        const uint4 r = k < end ? j.rec[k] : make_uint4(UNTS_SKIP, 0u, 0u, 0u);
        if (fault) {  // (the same in every lane)
            if (k < end) j.piece[k] = make_uint4(0u, 0u, 0u, 0u);
            continue;
        }
        const uint32_t kind = r.x & 15u, pusi = (r.x >> 4) & 1u, cc = (r.x >> 8) & 15u;
        const bool pay = kind >= UNTS_PAY;
        const unsigned long long m = __ballot(pay), mp = __ballot(kind == UNTS_PAY && pusi);
        const int prev = (m & lt) ? 63 - __clzll((long long)(m & lt)) : -1;
        const uint32_t pcc = __shfl(cc, prev < 0 ? 0 : prev);
        const int32_t want = prev >= 0 ? (int32_t)((pcc + 1u) & 15u) : expect;
        const bool open_here = open || (mp & lt) != 0ull;
        int32_t f = 0;
        if (kind == UNTS_BAD)
            f = 2;
        else if (pay && want >= 0 && (int32_t)cc != want)
            f = 3;
        else if (pay && (kind == UNTS_BAD_PES || (!pusi && !open_here)))
            f = 2;
        const unsigned long long mf = __ballot(f != 0);
        const int first = mf ? __ffsll((long long)mf) - 1 : 64;
        const unsigned long long front = first < 64 ? (1ull << first) - 1ull : ~0ull;
        const uint32_t n = (pay && lane < first) ? r.y : 0u;
        const uint32_t incl = wave_scan(n, lane, ScanAdd()), at = w + incl - n;
        if (k < end) {
            const unsigned long long src = ((unsigned long long)r.w << 32 | r.z) + (r.x >> 16);
            j.piece[k] = n ? make_uint4((uint32_t)src, (uint32_t)(src >> 32), n | (uint32_t)s << 8, at) : make_uint4(0u, 0u, 0u, 0u);
        }
        if (mp & front) {  // the last PES packet that begins in front of the fault
            pes_w = __shfl(at, 63 - __clzll((long long)(mp & front)));
            open = true;
        }
        if (m & front) expect = (int32_t)((__shfl(cc, 63 - __clzll((long long)(m & front))) + 1u) & 15u);
        w += __shfl(incl, 63);
        if (first < 64) fault = __shfl(f, first);
    }
    if (fault && open) w = pes_w;
    if (lane == 0) {
        j.res[s] = (int32_t)w;
        j.res[j.S + s] = fault;
        j.res[2 * j.S + s] = fault ? -1 : expect;
    }
}

// 16 lanes per packet: lane l takes the 16-byte word l of the destination that the piece touches; a word the piece fills is
// put together from byte loads (the source has any alignment and is read inside the packet only) and stored whole, the
// words at the two ends byte-wise.  A piece has at most 184 bytes: 13 words.
__global__ __launch_bounds__(256) void k_unts_gather(FerUntsJob j)
{
    const uint32_t k = blockIdx.x * 16u + (threadIdx.x >> 4), l = threadIdx.x & 15u;
    if (k >= j.npk) return;
    const uint4 pc = j.piece[k];
    const int n = (int)(pc.z & 255u);
    if (n == 0) return;
    const uint8_t *src = j.base + ((unsigned long long)pc.y << 32 | pc.x);
    uint8_t *dst = j.stage + j.sbase[pc.z >> 8] + pc.w;
    const int lo = (int)(l * 16u) - (int)((uintptr_t)dst & 15u), hi = lo + 16;
    if (lo >= n) return;
    if (lo >= 0 && hi <= n) {
        uint32_t q[4];
#pragma unroll
        for (int i = 0; i < 4; i++)
            q[i] = (uint32_t)src[lo + 4 * i] | (uint32_t)src[lo + 4 * i + 1] << 8 | (uint32_t)src[lo + 4 * i + 2] << 16 | (uint32_t)src[lo + 4 * i + 3] << 24;
        *(uint4 *)(dst + lo) = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
        for (int i = max(lo, 0); i < min(hi, n); i++) dst[i] = src[i];
    }
}

int fer_unts_run(FerUnts &u, hipStream_t st, const uint8_t *d_base, const ferhip_ts_run *runs, size_t nruns, const uint32_t *first, int S,
                 const uint16_t *pids, int32_t *expect, int32_t *fault)
{
    u.ptrs.assign(S, nullptr);
    u.lens.assign(S, 0);
    for (int s = 0; s < S; s++) fault[s] = 0;
    unsigned long long npk = 0;
    for (size_t r = 0; r < nruns; r++) npk += runs[r].bytes / TS_PKT;
    if (npk == 0) return 0;
    if (npk > 0x7fffffffull || nruns > 0x7fffffffull || S >= (1 << 24)) return FERHIP_E_ARG;
    // job words: sfirst[S + 1], pids[S], expectation[S], pfirst[nruns + 1], then the staging bases as 64-bit values
    const size_t words = ((size_t)(3 * S + 1) + nruns + 1 + 1) & ~(size_t)1;
    const size_t jw = words + 2 * (size_t)S;
    if (u.d_runs.reserve(nruns, nruns + nruns / 4) || u.h_runs.reserve(nruns, nruns + nruns / 4) || u.d_rec.reserve(npk, npk + npk / 4) ||
        u.d_piece.reserve(npk, npk + npk / 4) || u.d_job.reserve(jw, jw + jw / 4) || u.h_job.reserve(jw, jw + jw / 4) ||
        u.d_res.reserve(3 * (size_t)S) || u.h_res.reserve(3 * (size_t)S))
        return FERHIP_E_HIP;
    memcpy(u.h_runs, runs, nruns * sizeof(ferhip_ts_run));
    uint32_t *hj = u.h_job;
    uint32_t *pf = hj + 3 * S + 1;
    unsigned long long *hb = (unsigned long long *)(hj + words);
    uint32_t at = 0;
    for (size_t r = 0; r < nruns; r++) {
        pf[r] = at;
        at += runs[r].bytes / TS_PKT;
    }
    pf[nruns] = at;
    unsigned long long total = 0;
    for (int s = 0; s < S; s++) {
        hj[s] = pf[first[s]];
        hj[S + 1 + s] = pids[s];
        hj[2 * S + 1 + s] = (uint32_t)expect[s];
        hb[s] = total;
        // a packet stages at most 184 bytes
        total += ((unsigned long long)(pf[first[s + 1]] - pf[first[s]]) * 184ull + 16ull + 15ull) & ~15ull;
    }
    hj[S] = at;
    if (u.d_stage.reserve((size_t)total, (size_t)(total + total / 4))) return FERHIP_E_HIP;
    CK(hipMemcpyAsync(u.d_runs, u.h_runs, nruns * sizeof(ferhip_ts_run), hipMemcpyHostToDevice, st));
    CK(hipMemcpyAsync(u.d_job, u.h_job, jw * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    FerUntsJob j;
    j.base = d_base;
    j.runs = u.d_runs;
    j.pfirst = u.d_job.p + 3 * S + 1;
    j.nruns = (uint32_t)nruns;
    j.npk = (uint32_t)npk;
    j.S = S;
    j.rec = u.d_rec;
    j.piece = u.d_piece;
    j.sfirst = u.d_job;
    j.pids = u.d_job.p + S + 1;
    j.expect = (const int32_t *)(u.d_job.p + 2 * S + 1);
    j.sbase = (const unsigned long long *)(u.d_job.p + words);
    j.res = u.d_res;
    j.stage = u.d_stage;
    hipLaunchKernelGGL(k_unts_parse, dim3((unsigned)((npk + 255) / 256)), dim3(256), 0, st, j);
    hipLaunchKernelGGL(k_unts_walk, dim3(S), dim3(64), 0, st, j);
    hipLaunchKernelGGL(k_unts_gather, dim3((unsigned)((npk + 15) / 16)), dim3(256), 0, st, j);
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

// known-answer surface of the way in: host packets through the same kernels and the splitter, on the null stream
extern "C" int ferhip_unts_blocks(const uint8_t *base, size_t base_bytes, const ferhip_ts_run *runs, size_t nruns, int nstreams, int misalign,
                                  const uint16_t *pids, const int32_t *cc_expect, uint8_t *out, size_t cap, ferhip_nal_unit *units,
                                  size_t units_cap, size_t *nunits, int32_t *fault, int32_t *cc_next)
{
    if (nunits) *nunits = 0;
    if (!nunits || !fault || !cc_next || !cc_expect || !pids || nstreams <= 0 || nstreams > 65535 || misalign < 0 || misalign > 15 ||
        (!out && cap) || (!units && units_cap) || (nruns && (!base || !runs)))
        return FERHIP_E_ARG;
    for (size_t k = 0; k < nruns; k++)
        if (runs[k].offset > base_bytes || runs[k].bytes > base_bytes - runs[k].offset || runs[k].bytes % TS_PKT) return FERHIP_E_ARG;
    for (int s = 0; s < nstreams; s++)
        if (pids[s] > 0x1FFF || cc_expect[s] < -1 || cc_expect[s] > 15) return FERHIP_E_ARG;
    std::vector<ferhip_ts_run> sorted;
    std::vector<uint32_t> first;
    if (fer_rtp_sort(runs, nruns, nstreams, sorted, first)) return FERHIP_E_ARG;
    DevBuf<uint8_t> dbase, dst;
    FerUnts u;
    FerSplit sp;
    if (dbase.reserve((size_t)misalign + std::max<size_t>(base_bytes, 1)) || dst.reserve(std::max<size_t>(cap, 16))) return FERHIP_E_HIP;
    if (base_bytes) CK(hipMemcpy(dbase + misalign, base, base_bytes, hipMemcpyHostToDevice));
    if (cap) CK(hipMemcpy(dst, out, cap, hipMemcpyHostToDevice));
    for (int s = 0; s < nstreams; s++) cc_next[s] = cc_expect[s];
    if (int rc = fer_unts_run(u, nullptr, dbase + misalign, sorted.data(), nruns, first.data(), nstreams, pids, cc_next, fault)) return rc;
    size_t staged = 0;
    for (size_t n : u.lens) staged += n;
    if (!staged) return 0;  // no byte at all: nothing for the splitter
    if (int rc = fer_split_run(sp, nullptr, u.ptrs.data(), u.lens.data(), nstreams, dst, cap, 0)) return rc;
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
