// fer_dec_session.h -- the decode session (fer_dec_session.hip) that ferhip_decode_streams, the streaming decoder
// (fer_decode_host.hip) and the live decoder (fer_decode_live.hip) share: a decode-only context and windows of pictures.
#pragma once
#include "fer_ctx.h"
#include "fer_dec_syntax_host.h"
#include "fer_pic_host.h"
#include <chrono>
#include <thread>

#pragma GCC visibility push(hidden)

static inline double dec_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// f(i) for every i < items, item i on thread i % threads; inline when threads <= 1
template <typename F>
static void dec_fan_out(size_t items, size_t threads, F f)
{
    if (threads <= 1) {
        for (size_t i = 0; i < items; i++) f(i);
        return;
    }
    std::vector<std::thread> th;
    for (size_t k = 0; k < threads; k++)
        th.emplace_back([=, &f]() {
            for (size_t i = k; i < items; i += threads) f(i);
        });
    for (auto &x : th) x.join();
}
// host work per stream (splitting, gathering) is spread over a few threads
static inline size_t dec_stream_threads(int S) { return (size_t)std::max(1, std::min(std::min(S, 16), (int)std::thread::hardware_concurrency())); }

// the three planes of stream s in a plane-major picture set ([S] Y, [S] Cb, [S] Cr)
struct PlaneSpans { size_t off[3], len[3]; };
static inline PlaneSpans dec_stream_planes(const FerDev &d, int s)
{
    const size_t S = (size_t)d.S;
    return {{(size_t)s * d.ysz, S * d.ysz + (size_t)s * d.csz, S * (d.ysz + d.csz) + (size_t)s * d.csz}, {d.ysz, d.csz, d.csz}};
}

// Window buffers of the decode twin.  ferhip_decode_streams keeps one arena per process between calls (releasing
// tens of GB costs more than a window's reconstruction); it is tied to the HIP device it was allocated on and
// can be dropped with ferhip_decode_release().  A streaming decoder owns a small one of its own.  Freed on its device.
struct DecArena {
    DevBuf<uint8_t> dev;
    int device = -1;
    DevBuf<uint8_t> d_rbsp;  // slices of a window: device buffer ...
    PinBuf<uint8_t> h_rbsp;  // ... and pinned staging
    bool busy = false, cached = false;
};

// One decoding session: S streams of one picture size, a window of up to TWmax pictures per stream parsed by one
// launch, parameter sets and the state the reference keeps in globals (mb_qp_delta, ChromaACLevel) per stream.
struct DecSession {
    ferhip_ctx *c = nullptr;
    int S = 0;
    std::vector<DecHdr> hs;  // parameter sets of every stream (the QP of this codec lives in the PPS)
    DecArena *ar = nullptr;
    DecBatch B;
    uint32_t *d_info = nullptr;
    size_t TWmax = 0, nm = 0, fsz = 0;
    std::vector<uint32_t> info, hdr;
    std::vector<char> anyP, anyAny, keep, pres;  // pres[t * S + s]: stream s has a picture at step t of the window
    // A picture whose slice carries an empty reference-list modification is NOT stored as the reference picture
    // (modificationProcess, F/ref_frames.cpp:130-183): the stream's last decoded picture (what `frame` holds, what a
    // slice that ends early leaves in place) then differs from its reference picture and waits in `hold`.
    DevBuf<uint8_t> hold;
    std::vector<char> held;
    double t_pack = 0, t_parse = 0, t_recon = 0;
    const uint8_t *dev_rbsp = nullptr;  // the device splitter's store: where the `dev` units of a window lie
    std::vector<uint8_t> whole;         // a device unit whose slice header runs past its prefix, fetched to be parsed again
};

// Where the pictures of a window go.  rows (ferhip_decode_streams, ferhip_dec_nal): whole pictures in host memory, picture t
// of stream s at (t * S + s) * fsz, read back by ferhip_get_recon when every stream has one at a step, else plane by plane.
// Else slots (the live decoder): picture k of stream s in slot k * S + s, in device memory or staged for host memory.
struct DecOutput {
    uint8_t *out = nullptr;      // NULL: the pictures go nowhere
    bool rows = false;           // whole pictures in host memory
    bool out_dev = false;        // slots: out is device memory
    DevBuf<int2> d_map;          // [TWmax][S] device: the (stream, slot) pairs of every step for the output kernel
    std::vector<int2> map;       // ... host side
    std::vector<int> nmap;       // [TW] pairs per step
    std::vector<size_t> fin;     // host slots: slot (k * S + s) of the caller's buffer of every staged picture, in order
    DevBuf<uint8_t> d_stage;     // host slots: the window's pictures, packed, on the device ...
    PinBuf<uint8_t> h_stage;     // ... and pinned
    // ferhip_decs_set_display: the window (x0, y0, dw, dh) of every picture that goes to `out`; ofsz = bytes of one slot
    int win[4] = {};
    size_t ofsz = 0;
    // ferhip_decs_set_layout: the slots of device output are pitched I420 or NV12 (k_pic_emit) or a packed format
    // (k_pic_emit_packed); layout_set stays false on a decoder that never makes the call, and the slots are then tight I420
    bool layout_set = false;
    int fmt = FERHIP_FMT_I420;
    uint32_t pitch_y = 0, pitch_c = 0;
    int csc = FERHIP_CSC_BT601;  // ferhip_decs_set_csc: the matrix of a BGRA / RGBA layout
    uint32_t row_y() const { return layout_set ? pitch_y : (uint32_t)win[2]; }
    uint32_t row_c() const { return layout_set ? pitch_c : (uint32_t)win[2] / 2u; }
    // a layout other than tight I420 slots of the window: it needs device output and a check of its pitches
    bool own_layout() const { return !(fmt == FERHIP_FMT_I420 && row_y() == (uint32_t)win[2] && row_c() == (uint32_t)win[2] / 2u); }
    // whole coded pictures as tight I420 at a 16-byte aligned address: k_dec_out's case
    bool whole(const FerDev &d, const uint8_t *to) const { return !own_layout() && win[2] == d.W && win[3] == d.H && !((uintptr_t)to & 15u); }
    // plan: lays out the slots of the window's pictures (pictures[s] = those of stream s before it) and sends the map; emit:
    // the picture step t has just reconstructed; finish: waits for the stream, then the staged pictures go to the caller.
    int plan(DecSession &ss, size_t TW, const int *pictures);
    int emit(DecSession &ss, size_t t0, size_t t);
    int finish(DecSession &ss, size_t TW);
};

// Per-stream error isolation (the live decoder).  Without it the first stream that fails fails the window.  With it the
// faulted picture of a stream and its later ones are not reconstructed, status[s] records the FERHIP_E_*, the others go on.
struct DecIsolate {
    int *status = nullptr;   // [S] 0, or the first fault of stream s in this call
    std::vector<char> stop;  // [S] stream s faulted inside a window: it takes no more pictures in this call
};

// T = pictures per stream the caller expects (sizes the window); use_cache = take the process-wide arena.  A closed session
// can be opened again: open sets everything a window reads and clears the timers.
int dec_session_open(DecSession &ss, int W, int H, int S, size_t T, bool use_cache);
void dec_session_close(DecSession &ss);
// Decode pictures [t0, t0 + TW) of every stream: slices[s][t] = the slice NAL of picture t of stream s (streams may
// be shorter; nullptr = no picture at that step).  o receives them; pictures[s] counts (may be NULL).  iso: see DecIsolate.
int dec_session_window(DecSession &ss, const std::vector<std::vector<const NalRef *>> &slices, size_t t0, size_t TW, DecOutput &o,
                       int *pictures, DecIsolate *iso = nullptr);
// ferhip_decode_streams: the streams' RBSP, kept per calling thread until ferhip_decode_release
extern thread_local std::vector<std::vector<uint8_t>> tl_rbsp_store;

#pragma GCC visibility pop
