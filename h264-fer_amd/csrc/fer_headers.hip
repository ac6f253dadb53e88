// fer_headers.hip -- the host-written syntax above the macroblock layer: SPS and PPS (ferhip_write_sps / _pps /
// _pps_stream), writeNAL for host callers (ferhip_write_nal, F/nal.cpp:261-299) and each picture's slice header
// (build_header, F/headers_and_parameter_sets.cpp), whose bits go to the device as words for k_rc_plan and k_cavlc.
#include "fer_ctx.h"

// host bit writer (MSB first, F/rbsp_IO.cpp:123); bits past cap are counted, not stored
struct ByteW {
    uint8_t *b;
    size_t cap, nbits;
    void put(int k, unsigned x)
    {
        for (int i = k - 1; i >= 0; i--) {
            size_t by = nbits >> 3;
            if (by < cap) {
                if ((nbits & 7) == 0) b[by] = 0;
                b[by] |= (uint8_t)(((x >> i) & 1u) << (7 - (nbits & 7)));
            }
            nbits++;
        }
    }
    void ue(unsigned x)
    {
        int p = 0;
        while (((x + 1) >> (p + 1)) != 0) p++;
        put(p, 0);
        put(1, 1);
        if (p) put(p, x + 1 - (1u << p));
    }
    void se(int x) { ue(x <= 0 ? (unsigned)(-x) * 2u : (unsigned)x * 2u - 1u); }
    size_t trailing()
    {
        put(1, 1);
        while (nbits & 7) put(1, 0);
        return nbits >> 3;
    }
};

// sps_write, F/headers_and_parameter_sets.cpp:305-391
extern "C" size_t ferhip_write_sps(ferhip_ctx *c, uint8_t *rbsp, size_t cap)
{
    ByteW w{rbsp, cap, 0};
    w.put(8, 66);
    w.put(1, 1);
    w.put(1, 1);
    w.put(1, 0);
    w.put(5, 0);
    w.put(8, 41);
    w.ue(0);
    w.ue(5);  // log2_max_frame_num 9
    w.ue(0);
    w.ue(6);  // log2_max_pic_order_cnt_lsb 10
    w.ue(1);
    w.put(1, 0);
    w.ue((unsigned)(c->d.mbw - 1));
    w.ue((unsigned)(c->d.mbh - 1));
    w.put(1, 1);
    w.put(1, 1);
    if (c->disp_w < c->d.W || c->disp_h < c->d.H) {
        // frame_cropping_flag and the offsets left, right, top, bottom in units of two luma samples (4:2:0, frame_mbs_only);
        // the reference never crops, so this branch has no line of its own there
        w.put(1, 1);
        w.ue(0);
        w.ue((unsigned)(c->d.W - c->disp_w) / 2u);
        w.ue(0);
        w.ue((unsigned)(c->d.H - c->disp_h) / 2u);
    } else {
        w.put(1, 0);
    }
    w.put(1, 0);
    return w.trailing();
}

// pps_write, F/headers_and_parameter_sets.cpp:478-513 (weighted_bipred_idc field carries the value 1)
static size_t write_pps(int qp, uint8_t *rbsp, size_t cap)
{
    ByteW w{rbsp, cap, 0};
    w.ue(0);
    w.ue(0);
    w.put(1, 0);
    w.put(1, 0);
    w.ue(0);
    w.ue(0);
    w.ue(0);
    w.put(1, 0);
    w.put(2, 1);
    w.se(14 + qp - 26);
    w.se(0);
    w.se(0);
    w.put(1, 0);
    w.put(1, 0);
    w.put(1, 0);
    return w.trailing();
}

extern "C" size_t ferhip_write_pps(ferhip_ctx *c, uint8_t *rbsp, size_t cap) { return write_pps(c->p.qp, rbsp, cap); }

// the PPS of stream s: pic_init_qp = 14 + base[s] (0 for a bad argument)
extern "C" size_t ferhip_write_pps_stream(ferhip_ctx *c, int s, uint8_t *rbsp, size_t cap)
{
    if (!c || !rbsp || s < 0 || s >= c->d.S) return 0;
    return write_pps(c->rate[s].base, rbsp, cap);
}

// writeNAL, F/nal.cpp:261-299
extern "C" size_t ferhip_write_nal(int nal_ref_idc, int nal_type, const uint8_t *rbsp, size_t n, uint8_t *out)
{
    size_t pos = 0;
    out[pos++] = 0;
    out[pos++] = 0;
    out[pos++] = 0;
    out[pos++] = 1;
    out[pos++] = (uint8_t)((nal_ref_idc << 5) | (nal_type & 31));
    int zc = 0;
    for (size_t i = 0; i < n; i++) {
        if (zc >= 2 && rbsp[i] <= 3) {
            out[pos++] = 3;
            zc = 0;
        }
        out[pos++] = rbsp[i];
        zc = rbsp[i] == 0 ? zc + 1 : 0;
    }
    return pos;
}

// slice header of stream s for this picture: shd_write, F/headers_and_parameter_sets.cpp:172-239
void build_header(ferhip_ctx *c, int s, int nal_type)
{
    StreamState &t = c->ss[s];
    int slice_type;
    if (nal_type == FERHIP_NAL_NONE) {  // no picture of this stream in this call: its slice-level state stays
        c->h_hdr[s * 4 + 0] = c->h_hdr[s * 4 + 1] = c->h_hdr[s * 4 + 2] = 0;
        c->h_hdr[s * 4 + 3] = FER_PIC_ABSENT;
        c->types[s] = FER_PIC_ABSENT;
        return;
    }
    if (nal_type == FERHIP_NAL_IDR) {  // F/rbsp_encoding.cpp:142-164
        slice_type = 2;
        if (!t.first_idr_done) {
            t.first_idr_done = 1;
            t.idr_pic_id = 0;
        } else if (t.frame_num == 0) {
            t.idr_pic_id++;
        } else {
            t.idr_pic_id = 0;
        }
        t.frame_num = 0;
        t.poc_lsb = 0;
    } else {
        slice_type = 0;
        t.frame_num++;
        t.poc_lsb += 2;
    }
    uint8_t b[8] = {0};  // the header is a few dozen bits: it goes to the device as two words, right-aligned, and a bit count
    ByteW h{b, sizeof b, 0};
    h.ue(0);
    h.ue((unsigned)slice_type);
    h.ue(0);
    h.put(9, (unsigned)t.frame_num & 511u);
    if (nal_type == FERHIP_NAL_IDR) h.ue((unsigned)t.idr_pic_id);
    h.put(10, (unsigned)t.poc_lsb & 1023u);
    if (slice_type == 0) {
        h.put(1, 0);  // num_ref_idx_active_override_flag
        h.put(1, 0);  // ref_pic_list_modification_flag_l0
        h.put(1, 0);  // adaptive_ref_pic_marking_mode_flag
    } else {
        h.put(1, 0);  // no_output_of_prior_pics_flag
        h.put(1, 0);  // long_term_reference_flag
    }
    // slice_qp_delta is appended on the device by k_rc_plan once the picture's QP is known (fer_rate.hip)
    unsigned long long v = 0;
    for (int i = 0; i < 8; i++) v = v << 8 | b[i];
    v >>= 64 - h.nbits;
    c->h_hdr[s * 4 + 0] = (uint32_t)(v >> 32);
    c->h_hdr[s * 4 + 1] = (uint32_t)v;
    c->h_hdr[s * 4 + 2] = (uint32_t)h.nbits;
    c->h_hdr[s * 4 + 3] = (uint32_t)slice_type;
    c->types[s] = slice_type;
}
