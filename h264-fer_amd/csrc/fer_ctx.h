// fer_ctx.h -- the context of libferhip and the owners of its resources, for the host translation units that drive it
// (fer_api.hip, fer_headers.hip, fer_nalpack.hip, fer_rtp.hip, fer_ts.hip, fer_mp4.hip, fer_nalsplit.hip, fer_dec_session.hip, fer_decode_host.hip, fer_decode_live.hip, and
// fer_mbunit.hip, every buffer of which is a DevBuf).
#pragma once
#include "fer_internal.h"
#include <stdio.h>
#include <vector>

#pragma GCC visibility push(hidden)  // nothing here is part of the library's ABI

#define CK(x)                                                                                         \
    do {                                                                                              \
        hipError_t e_ = (x);                                                                          \
        if (e_ != hipSuccess) {                                                                       \
            fprintf(stderr, "ferhip: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return FERHIP_E_HIP;                                                                      \
        }                                                                                             \
    } while (0)

// One growable buffer of `cap` elements, in device memory or (PINNED) pinned host memory, and its only owner: it is freed
// with its holder.  reserve(need, want) keeps a buffer that holds `need` elements and otherwise allocates `want` (>= need;
// the caller's growth rule) afresh: what it held is not copied.  A failed allocation leaves it empty, with HIP's error cleared.
template <typename T, bool PINNED = false>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int reserve(size_t need, size_t want = 0)
    {
        if (cap >= need && (p || !need)) return 0;
        release();
        want = want > need ? want : need;
        if ((PINNED ? hipHostMalloc((void **)&p, want * sizeof(T)) : hipMalloc((void **)&p, want * sizeof(T))) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            return FERHIP_E_HIP;
        }
        cap = want;
        return 0;
    }
    void release()
    {
        if (p) PINNED ? (void)hipHostFree(p) : (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    operator T *() const { return p; }
};
template <typename T>
using PinBuf = DevBuf<T, true>;

// A ring of pinned slots that feed asynchronous copies.  A pinned source is read when the copy executes, not when it is
// enqueued, so a slot is rewritten only after the copy that last used it has run: next() waits for that copy's event,
// sent() records it.  A slot may carry a second payload behind the first (the header ring's rate settings): both ride on
// the slot's one event.
#define FER_HDR_SLOTS 8
struct PinnedRing {
    uint8_t *mem = nullptr;
    hipEvent_t ev[FER_HDR_SLOTS] = {};
    size_t slot_bytes = 0, second_off = 0;
    int slot = 0;
    int create(size_t bytes_per_slot, size_t second_bytes = 0);  // a call after a failed one creates only what is missing
    void *next();                                                // null when the wait fails
    void *second() const { return mem + (size_t)slot * slot_bytes + second_off; }
    int sent(hipStream_t st);
    void destroy();
};

struct StreamState {  // slice-level state of one stream (globals `shd`, statics of RBSP_encode)
    int frame_num, poc_lsb, idr_pic_id, first_idr_done, frames_done, have_dpb;
};

struct ferhip_ctx {
    FerDev d;
    ferhip_params p;
    hipStream_t st = nullptr;
    hipStream_t st_hi = nullptr;   // high-priority stream for the latency-bound per-diagonal chains
    hipStream_t st_aux = nullptr;  // the sort of the reference picture's positions runs here, beside k_me_pre (run_picture)
    hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_c = nullptr, ev_d = nullptr;
    // ferhip_tune: 1 / 2 = the HBM-bound sort is enqueued beside the VALU-bound stage-3 search (st_aux / st_hi).  Measured:
    // kernels of two HIP streams do not share the GPU here (the sort stretches to k_me_pre's length), so it is off
    int overlap_sort = 0;
    int device = 0;  // HIP device the context lives on; every entry point re-selects it (callers may use any thread)
    std::vector<StreamState> ss;
    // what the context owns until ferhip_destroy: device buffers (dalloc), pinned buffers (halloc), events (ealloc)
    std::vector<void *> allocs, pinned;
    std::vector<hipEvent_t> events;
    FerSortTmp sort = {};
    PinnedRing hdr_ring;        // [S][4] slice header words, then [S] FerRcPar: the rate settings go with the headers
    uint32_t *h_hdr = nullptr;  // the slot of the header ring that the picture in the making fills
    std::vector<FerRcPar> rate;  // ferhip_set_rate: the settings of every stream, sent with the next picture's headers
    bool rate_dirty = true;
    int qflags = 0;              // ferhip_set_quality
    long long q_count = 0;       // pictures measured so far: the next record goes to ring slot q_count % FERHIP_QUALITY_RING
    uint32_t *h_len = nullptr;   // pinned [S]
    int *h_status = nullptr;     // pinned [S]
    unsigned long long *h_sad = nullptr;
    std::vector<int> types;
    uint8_t *planes[2] = {};     // two picture sets, swapped after every picture
    // asynchronous ingest (ferhip_upload_frames): pinned host pictures -> stage[k] on a copy stream, double buffered
    hipStream_t st_copy = nullptr;
    uint8_t *stage[2] = {};
    hipEvent_t up_done[2] = {}, up_used[2] = {};
    int up_next = 0, up_ready = 0;  // slot the next upload fills; uploads waiting to be made current
    int cur_set = 0;
    bool refprep_valid = false;
    // display size (ferhip_set_display_size): the pictures are coded at W x H, the SPS crops them to disp_w x disp_h
    int disp_w = 0, disp_h = 0;
    bool coded = false;              // a picture has been coded: the display size is frozen
    bool up_disp[2] = {};            // the staging slot holds display-size pictures (ferhip_upload_frames_display)
    uint8_t *disp_stage = nullptr;   // ferhip_set_frames_display(host = 1): the pictures on their way to the pad kernel
    // live contexts: presence masks.  An ingest mask goes to the device through a pinned ring of its own; the mask of
    // k_frame_sad needs one slot only, because the read-back of the SADs waits for the stream
    uint8_t *d_present = nullptr, *d_sadskip = nullptr;  // device [S]
    PinnedRing pres_ring;                                // [S]
    uint8_t *h_sadskip = nullptr;                        // pinned [S]
    std::vector<uint8_t> up_mask[2];  // ferhip_upload_frames_live: the mask of each staging slot (empty = every stream)
    // pictures by descriptor (ferhip_set_pictures, ferhip_get_recon_pictures): the [S] table and its pinned ring, on first use
    ferhip_pic *d_pics = nullptr;  // device [S]
    PinnedRing pic_ring;           // [S] ferhip_pic
    int csc = FERHIP_CSC_BT601;    // ferhip_set_csc: the matrix of the BGRA / RGBA formats
    // NAL framing on the device (fer_nalpack.hip): everything is allocated on first use, the parameter set table and its
    // pinned ring only once FERHIP_AU_PARAM_SETS was asked for
    bool nal_ready = false;            // a picture call has been made: hdr and out_bytes describe a picture
    int nal_nchmax = 0;
    uint4 *nal_summ = nullptr;
    uint2 *nal_cin = nullptr, *nal_ent = nullptr;
    ferhip_au *nal_index = nullptr, *h_nal_index = nullptr;  // device / pinned [S + 1]: ferhip_fetch_nal's index
    uint8_t *nal_buf = nullptr;        // ferhip_fetch_nal's device buffer, regrown when a picture needs more (so not in allocs)
    size_t nal_buf_cap = 0;
    uint8_t *d_ps = nullptr;           // device [S][FER_NAL_PS_ROW]
    PinnedRing ps_ring;                // [S][FER_NAL_PS_ROW]
    std::vector<uint8_t> ps_dirty;     // [S] the stream's row must be sent (empty until the table exists)
    bool ps_wide = false;              // a row was too long to record where its PPS begins: no length-prefixed form
    // RTP packets (fer_rtp.hip), on first use: the callers' headers go to the device through a pinned ring of their own
    ferhip_rtp_au *rtp_index = nullptr, *h_rtp_index = nullptr;  // device / pinned [S + 1]: ferhip_fetch_rtp's index
    uint32_t *d_rtp_hdr = nullptr;     // device [S][3]: ferhip_rtp_hdr as three words
    PinnedRing rtp_ring;               // [S] ferhip_rtp_hdr
    DevBuf<uint8_t> rtp_buf;           // ferhip_fetch_rtp's packets and table on the device, regrown when a picture needs more
    DevBuf<ferhip_rtp_pkt> rtp_pkts;
    bool rtp_ready = false;            // the four above exist
    // transport stream packets (fer_ts.hip), on first use, as the RTP members above; the PSI table only once FERHIP_TS_PSI
    // was asked for
    ferhip_ts_au *ts_index = nullptr, *h_ts_index = nullptr;  // device / pinned [S + 1]: ferhip_fetch_ts's index
    ferhip_ts_hdr *d_ts_hdr = nullptr;  // device [S]
    PinnedRing ts_ring;                // [S] ferhip_ts_hdr
    DevBuf<uint8_t> ts_buf;            // ferhip_fetch_ts's packets on the device, regrown when a picture needs more
    bool ts_ready = false;             // the four above exist
    uint8_t *d_ts_psi = nullptr;       // device [S][376]: every stream's PAT and PMT packet
    PinnedRing ts_psi_ring;            // [S][376]
    std::vector<uint32_t> ts_psi_ids;  // [S] pid << 16 | pmt_pid of the stream's row, 0 = none yet (empty until the table exists)
    // fragmented MP4 segments (fer_mp4.hip), on first use.  The open segment's cursors are state[] on the device; the host
    // keeps only what it was given at open and whether the last picture has been appended
    uint4 *mp4_state = nullptr;                // device [S]: sample bytes, samples, fault, first sample's NAL unit type
    unsigned long long *mp4_place = nullptr;   // device [S]: where the append in flight puts each stream's sample
    ferhip_mp4_hdr *d_mp4_hdr = nullptr;       // device [S]
    ferhip_mp4_seg *mp4_index = nullptr, *h_mp4_index = nullptr;  // device / pinned [S + 1]: ferhip_mp4_fetch's index
    PinnedRing mp4_ring;                       // [S] ferhip_mp4_hdr
    bool mp4_ready = false;                    // the six above exist
    bool mp4_open = false, mp4_appended = false;
    uint8_t *mp4_dst = nullptr;                // the open segment: the caller's regions, K and flags
    size_t mp4_stride = 0;
    int mp4_K = 0, mp4_flags = 0;
    unsigned long long pic_serial = 0, mp4_serial = 0;  // picture calls made; the one the last append took
    // live kernel timing with HIP events on the launch stream (bench.py roofline leg)
    bool prof = false;
    struct Span { int phase; hipEvent_t a, b; long launches; };
    std::vector<Span> spans;
    double prof_ms[FERHIP_NPHASE] = {};
    long prof_launches[FERHIP_NPHASE] = {};
};

struct ProfScope {
    ferhip_ctx *c;
    int idx;
    hipStream_t s;
    ProfScope(ferhip_ctx *c_, int phase, long launches, hipStream_t s_ = nullptr) : c(c_), idx(-1), s(s_ ? s_ : c_->st)
    {
        if (!c->prof) return;
        ferhip_ctx::Span sp{phase, nullptr, nullptr, launches};
        hipEventCreate(&sp.a);
        hipEventCreate(&sp.b);
        hipEventRecord(sp.a, s);
        c->spans.push_back(sp);
        idx = (int)c->spans.size() - 1;
    }
    ~ProfScope()
    {
        if (idx >= 0) hipEventRecord(c->spans[idx].b, s);
    }
};

// The three allocators hand the resource to the context, which frees it in ferhip_destroy.  *p that is already set is kept:
// a lazy set-up that failed half way allocates only what is still missing when it is called again.
template <typename T>
static int dalloc(ferhip_ctx *c, T **p, size_t n)  // device, cleared (on the null stream)
{
    if (*p) return 0;
    void *v = nullptr;
    if (hipMalloc(&v, n * sizeof(T) + 256) != hipSuccess) return FERHIP_E_HIP;
    c->allocs.push_back(v);
    if (hipMemset(v, 0, n * sizeof(T) + 256) != hipSuccess) return FERHIP_E_HIP;
    *p = (T *)v;
    return 0;
}
template <typename T>
static int halloc(ferhip_ctx *c, T **p, size_t n)  // pinned host
{
    if (*p) return 0;
    void *v = nullptr;
    if (hipHostMalloc(&v, n * sizeof(T)) != hipSuccess) return FERHIP_E_HIP;
    c->pinned.push_back(v);
    *p = (T *)v;
    return 0;
}
int ealloc(ferhip_ctx *c, hipEvent_t *e);  // event without timing

// decode_only: the encoder-side structures (interpolated planes, features, sort, search lists, RBSP) stay empty
int ctx_create(ferhip_ctx **out, int W, int H, int S, const ferhip_params *p, bool decode_only);
void bind_planes(ferhip_ctx *c);  // FerDev's cur / ref plane pointers from cur_set
// slice header of stream s for this picture into c->h_hdr (fer_headers.hip); nal_type FERHIP_NAL_NONE = no picture
void build_header(ferhip_ctx *c, int s, int nal_type);

#pragma GCC visibility pop
