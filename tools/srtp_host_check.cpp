// The host half of SRTP (h264-fer_amd/csrc/fer_srtp_host.h) as a stand-alone program, for a run under a sanitizer:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/srtp_host_check.cpp -o srtp_host_check && ./srtp_host_check
// Every input is a heap array of exactly its length, so a reader that leaves what it was given is an error.
// Without arguments it checks the published vectors (FIPS-197 C.1, RFC 3711 B.2 and B.3, RFC 2202 case 1), the header rule
// on every truncation of dressed headers (CC 0..15, with and without an extension) against the rule written out a second
// time, the index estimate's hand cases and the refusals.
//   srtp_host_check list FILE
// checks a listing, one record a line, fields in hex unless noted (tests/test_srtp_host_check.py writes it from
// tests/golden/srtp_kat.json and tests/srtp_model.py):
//   ecb KEY IN OUT | ctr KEY IV OUT | hmac KEY20 MSG OUT | derive MKEY MSALT KE KA KS | row MKEY MSALT ROUNDKEYS MID_I MID_O
//   hdr PACKET hl(decimal) | est roc s_l seq v (decimal) | protect MKEY MSALT roc s_l(decimal) PACKET SRTP
// and prints the number of records; any difference is reported and the exit status is 1.
//   srtp_host_check rate NPACKETS BYTES
// protects NPACKETS packets of BYTES bytes on this core (the whole host route: counter mode keystream, XOR, HMAC-SHA1 tag)
// and prints the seconds it took: what tools/srtp_rate.py compares the device with.
#include "../h264-fer_amd/csrc/fer_srtp_host.h"
#include <stdio.h>
#include <stdlib.h>
#include <chrono>
#include <memory>
#include <string>
#include <vector>

typedef std::vector<uint8_t> Bytes;
static int fails = 0;
#define EXPECT(x)                                              \
    do {                                                       \
        if (!(x)) {                                            \
            printf("line %d: %s\n", __LINE__, #x);             \
            fails++;                                           \
        }                                                      \
    } while (0)

static uint32_t tab[FER_SRTP_TAB];

static Bytes hex(const std::string &s)
{
    Bytes b;
    if (s == "-") return b;
    for (size_t i = 0; i + 1 < s.size(); i += 2) b.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return b;
}

// a heap copy of exactly the bytes' length
struct Exact {
    std::unique_ptr<uint8_t[]> p;
    size_t n;
    explicit Exact(const Bytes &b) : p(new uint8_t[b.size()]), n(b.size())
    {
        if (n) memcpy(p.get(), b.data(), n);
    }
    const uint8_t *get() const { return p.get(); }
};

static Bytes ecb(const Bytes &key, const Bytes &in)
{
    uint32_t rk[44];
    fer_aes_expand(tab, Exact(key).get(), rk);
    Exact src(in);
    Bytes out(in.size());
    for (size_t i = 0; i + 16 <= in.size(); i += 16) fer_aes_block_bytes(tab, rk, src.get() + i, out.data() + i);
    return out;
}

static Bytes ctr(const Bytes &key, const Bytes &iv, size_t n)
{
    uint32_t rk[44];
    fer_aes_expand(tab, Exact(key).get(), rk);
    std::unique_ptr<uint8_t[]> out(new uint8_t[n ? n : 1]);
    fer_aes_cm(tab, rk, Exact(iv).get(), out.get(), n);
    return Bytes(out.get(), out.get() + n);
}

static Bytes mac(const Bytes &key20, const Bytes &msg)
{
    uint32_t mi[5], mo[5];
    Exact k(key20), m(msg);
    fer_hmac_midstate(k.get(), 0x36, mi);
    fer_hmac_midstate(k.get(), 0x5c, mo);
    Bytes out(20);
    fer_hmac_sha1(mi, mo, m.get(), m.n, out.data());
    return out;
}

// The whole host route for one packet: what a sender without the device pass does.  state = (roc, s_l) with set = 1.
static Bytes protect(const uint32_t row[FER_SRTP_ROW], uint32_t roc, uint32_t s_l, const Bytes &pkt)
{
    Exact p(pkt);
    const uint32_t L = (uint32_t)p.n, hl = fer_srtp_header(p.get(), L);
    if (!hl) return Bytes();
    const uint32_t seq = (uint32_t)p.get()[2] << 8 | p.get()[3], ssrc = fer_be32(p.get() + 8);
    const uint32_t v = fer_srtp_estimate(roc, s_l, seq);
    uint8_t iv[16];
    fer_put_be32(iv, row[FER_SRTP_ROW_KS]);
    fer_put_be32(iv + 4, row[FER_SRTP_ROW_KS + 1] ^ ssrc);
    fer_put_be32(iv + 8, row[FER_SRTP_ROW_KS + 2] ^ v);
    fer_put_be32(iv + 12, row[FER_SRTP_ROW_KS + 3] ^ seq << 16);
    Bytes out(L + 4);
    memcpy(out.data(), p.get(), L);
    std::unique_ptr<uint8_t[]> ks(new uint8_t[L - hl ? L - hl : 1]);
    fer_aes_cm(tab, row, iv, ks.get(), L - hl);
    for (uint32_t i = hl; i < L; i++) out[i] ^= ks[i - hl];
    fer_put_be32(out.data() + L, v);
    uint8_t t[20];
    fer_hmac_sha1(row + FER_SRTP_ROW_MID_I, row + FER_SRTP_ROW_MID_O, out.data(), L + 4, t);
    out.resize(L);
    out.insert(out.end(), t, t + FER_SRTP_TAG);
    return out;
}

// the header rule, written out a second time over a vector with bounds-checked reads
static uint32_t header_again(const Bytes &p)
{
    const size_t L = p.size();
    if (L < 12) return 0;
    if ((p.at(0) & 0xC0) != 0x80) return 0;
    size_t hl = 12 + 4 * (size_t)(p.at(0) & 15);
    if (p.at(0) & 0x10) {
        if (hl + 4 > L) return 0;
        hl += 4 + 4 * ((size_t)p.at(hl + 2) * 256 + p.at(hl + 3));
    }
    if (hl > L || L - hl > FER_SRTP_MAX_PAYLOAD) return 0;
    return (uint32_t)hl;
}

static void self_check()
{
    EXPECT(ecb(hex("000102030405060708090a0b0c0d0e0f"), hex("00112233445566778899aabbccddeeff")) == hex("69c4e0d86a7b0430d8cdb78070b4c55a"));
    EXPECT(ctr(hex("2B7E151628AED2A6ABF7158809CF4F3C"), hex("F0F1F2F3F4F5F6F7F8F9FAFBFCFD0000"), 48) ==
           hex("E03EAD0935C95E80E166B16DD92B4EB4D23513162B02D0F72A43A2FE4A5F97AB41E95B3BB0A2E8DD477901E4FCA894C0"));
    EXPECT(ctr(hex("2B7E151628AED2A6ABF7158809CF4F3C"), hex("F0F1F2F3F4F5F6F7F8F9FAFBFCFDFEFF"), 48) ==
           hex("EC8CDF7398607CB0F2D21675EA9EA1E4362B7C3C6773516318A077D7FC5073AE6A2CC3787889374FBEB4C81B17BA6C44"));
    {
        Exact mk(hex("E1F97A0D3E018BE0D64FA32C06DE4139")), ms(hex("0EC675AD498AFEEBB6960B3AABE6"));
        std::unique_ptr<uint8_t[]> k(new uint8_t[50]);
        fer_srtp_derive(tab, mk.get(), ms.get(), k.get());
        EXPECT(Bytes(k.get(), k.get() + 16) == hex("C61E7A93744F39EE10734AFE3FF7A087"));
        EXPECT(Bytes(k.get() + 16, k.get() + 36) == hex("CEBE321F6FF7716B6FD4AB49AF256A156D38BAA4"));
        EXPECT(Bytes(k.get() + 36, k.get() + 50) == hex("30CBBC08863D8C85D49DB34A9AE1"));
    }
    EXPECT(mac(Bytes(20, 0x0b), Bytes{'H', 'i', ' ', 'T', 'h', 'e', 'r', 'e'}) == hex("b617318655057264e28bc0b6fb378c8ef146be00"));
    // the header rule on every truncation of dressed headers
    for (unsigned cc = 0; cc < 16; cc++)
        for (int ext = -1; ext <= 3; ext++)
            for (unsigned version = 1; version <= 3; version++) {
                Bytes p = {(uint8_t)(version << 6 | (ext >= 0 ? 0x10 : 0) | cc), 96, 0x12, 0x34, 1, 2, 3, 4, 5, 6, 7, 8};
                p.insert(p.end(), 4 * cc, 0xC5);
                if (ext >= 0) {
                    const uint8_t h[4] = {0xBE, 0xDE, (uint8_t)(ext >> 8), (uint8_t)ext};
                    p.insert(p.end(), h, h + 4);
                    p.insert(p.end(), 4 * (size_t)ext, 0xE7);
                }
                const size_t full = p.size();
                p.insert(p.end(), 5, 0x99);
                for (size_t n = 0; n <= p.size(); n++) {
                    const Bytes cut(p.begin(), p.begin() + n);
                    Exact e(cut);
                    const uint32_t hl = fer_srtp_header(e.get(), (uint32_t)e.n);
                    EXPECT(hl == header_again(cut));
                    EXPECT(hl == (version == 2 && n >= full ? full : 0));
                }
            }
    {  // a payload of 2^20 bytes stands, one byte more does not
        Bytes p(12 + FER_SRTP_MAX_PAYLOAD + 1, 0);
        p[0] = 0x80;
        EXPECT(fer_srtp_header(p.data(), (uint32_t)p.size() - 1) == 12 && fer_srtp_header(p.data(), (uint32_t)p.size()) == 0);
    }
    static const uint32_t hand[6][4] = {{0, 65535, 0, 1}, {1, 2, 65534, 0}, {0, 0, 32768, 0}, {0, 0, 32769, 0xFFFFFFFFu}, {5, 32768, 0, 5}, {5, 32769, 0, 6}};
    for (const auto &h : hand) EXPECT(fer_srtp_estimate(h[0], h[1], h[2]) == h[3]);
    // the refusals
    {
        const uint8_t keyed[3] = {1, 0, 1};
        std::unique_ptr<FerSrtpRow[]> rows(new FerSrtpRow[2]);
        rows[0] = {0, 40, 0};
        rows[1] = {48, 40, 2};
        EXPECT(fer_srtp_check_rows(rows.get(), 2, 3, keyed, ~0ull) == 0);
        EXPECT(fer_srtp_check_rows(rows.get(), 2, 3, keyed, 88) == 0 && fer_srtp_check_rows(rows.get(), 2, 3, keyed, 87) == -1);
        EXPECT(fer_srtp_check_rows(rows.get(), 2, 2, keyed, ~0ull) == -1);
        EXPECT(fer_srtp_check_rows(nullptr, 2, 3, keyed, ~0ull) == -1 && fer_srtp_check_rows(nullptr, 0, 3, keyed, ~0ull) == 0);
        rows[1].stream = 1;
        EXPECT(fer_srtp_check_rows(rows.get(), 2, 3, keyed, ~0ull) == -3);
        rows[0].stream = 3;  // a stream out of range comes before a key that is missing
        EXPECT(fer_srtp_check_rows(rows.get(), 2, 3, keyed, ~0ull) == -1);
        rows[0] = {~0ull - 3, 40, 0};
        EXPECT(fer_srtp_check_rows(rows.get(), 1, 3, keyed, 1000) == -1);
        alignas(16) static uint8_t buf[32];
        EXPECT(fer_srtp_check_out(buf, 32, buf, 16, 8) == 0 && fer_srtp_check_out(buf + 8, 8, buf, 16, 8) == -1);
        EXPECT(fer_srtp_check_out(buf, 32, buf + 4, 16, 8) == -1 && fer_srtp_check_out(buf, 32, nullptr, 16, 8) == -1);
        EXPECT(fer_srtp_check_out(nullptr, 1, buf, 16, 8) == -1 && fer_srtp_check_out(nullptr, 0, buf, 16, 8) == 0);
        EXPECT(fer_srtp_check_out(buf + 1, 8, buf + 1, 1, 1) == 0);
    }
}

static std::vector<std::string> fields(const char *line)
{
    std::vector<std::string> f;
    std::string cur;
    for (const char *c = line; *c; c++) {
        if (*c == ' ' || *c == '\n' || *c == '\r') {
            if (!cur.empty()) f.push_back(cur);
            cur.clear();
        } else
            cur += *c;
    }
    if (!cur.empty()) f.push_back(cur);
    return f;
}

static int list_check(const char *path)
{
    FILE *fp = fopen(path, "r");
    if (!fp) {
        printf("cannot open %s\n", path);
        return 2;
    }
    std::vector<char> line(1 << 22);
    long n = 0;
    while (fgets(line.data(), (int)line.size(), fp)) {
        const std::vector<std::string> f = fields(line.data());
        if (f.empty()) continue;
        n++;
        bool ok = false;
        if (f[0] == "ecb" && f.size() == 4)
            ok = ecb(hex(f[1]), hex(f[2])) == hex(f[3]);
        else if (f[0] == "ctr" && f.size() == 4)
            ok = ctr(hex(f[1]), hex(f[2]), hex(f[3]).size()) == hex(f[3]);
        else if (f[0] == "hmac" && f.size() == 4)
            ok = mac(hex(f[1]), hex(f[2])) == hex(f[3]);
        else if ((f[0] == "derive" && f.size() == 6) || (f[0] == "row" && f.size() == 6) || (f[0] == "protect" && f.size() == 7)) {
            Exact mk(hex(f[1])), ms(hex(f[2]));
            if (mk.n != 16 || ms.n != 14) {
                ok = false;
            } else if (f[0] == "derive") {
                std::unique_ptr<uint8_t[]> k(new uint8_t[50]);
                fer_srtp_derive(tab, mk.get(), ms.get(), k.get());
                Bytes want = hex(f[3]), ka = hex(f[4]), ks = hex(f[5]);
                want.insert(want.end(), ka.begin(), ka.end());
                want.insert(want.end(), ks.begin(), ks.end());
                ok = Bytes(k.get(), k.get() + 50) == want;
            } else {
                std::unique_ptr<uint32_t[]> row(new uint32_t[FER_SRTP_ROW]);
                fer_srtp_row(tab, mk.get(), ms.get(), row.get());
                if (f[0] == "row") {
                    Bytes got(176 + 40);
                    for (int i = 0; i < 44; i++) fer_put_be32(got.data() + 4 * i, row[i]);
                    for (int i = 0; i < 10; i++) fer_put_be32(got.data() + 176 + 4 * i, row[FER_SRTP_ROW_MID_I + i]);
                    Bytes want = hex(f[3]), mi = hex(f[4]), mo = hex(f[5]);
                    want.insert(want.end(), mi.begin(), mi.end());
                    want.insert(want.end(), mo.begin(), mo.end());
                    ok = got == want && row[FER_SRTP_ROW_KEYED] == 1;
                } else
                    ok = protect(row.get(), (uint32_t)strtoul(f[3].c_str(), nullptr, 10), (uint32_t)strtoul(f[4].c_str(), nullptr, 10), hex(f[5])) == hex(f[6]);
            }
        } else if (f[0] == "hdr" && f.size() == 3) {
            Exact p(hex(f[1]));
            ok = fer_srtp_header(p.get(), (uint32_t)p.n) == strtoul(f[2].c_str(), nullptr, 10);
        } else if (f[0] == "est" && f.size() == 5)
            ok = fer_srtp_estimate((uint32_t)strtoul(f[1].c_str(), nullptr, 10), (uint32_t)strtoul(f[2].c_str(), nullptr, 10),
                                   (uint32_t)strtoul(f[3].c_str(), nullptr, 10)) == strtoul(f[4].c_str(), nullptr, 10);
        if (!ok) {
            printf("record %ld (%s) differs\n", n, f[0].c_str());
            fails++;
        }
    }
    fclose(fp);
    printf("%ld records\n", n);
    return fails ? 1 : 0;
}

static int rate(long npackets, long bytes)
{
    if (npackets <= 0 || bytes < 12 || bytes > 65535) return 2;
    const uint8_t mk[16] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}, ms[14] = {21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34};
    uint32_t row[FER_SRTP_ROW];
    fer_srtp_row(tab, mk, ms, row);
    Bytes p((size_t)bytes, 0x5A);
    p[0] = 0x80;
    unsigned sink = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (long k = 0; k < npackets; k++) {
        p[2] = (uint8_t)(k >> 8), p[3] = (uint8_t)k;
        const Bytes out = protect(row, (uint32_t)(k >> 16), (uint32_t)(k ? (k - 1) & 0xffff : 0), p);
        sink += out.back();
    }
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("%.6f seconds %ld packets %ld bytes (%u)\n", s, npackets, bytes, sink & 1u);
    return 0;
}

int main(int argc, char **argv)
{
    fer_aes_tables(tab);
    if (argc == 3 && std::string(argv[1]) == "list") return list_check(argv[2]);
    if (argc == 4 && std::string(argv[1]) == "rate") return rate(atol(argv[2]), atol(argv[3]));
    if (argc != 1) {
        printf("usage: srtp_host_check [list FILE | rate NPACKETS BYTES]\n");
        return 2;
    }
    self_check();
    printf(fails ? "%d checks failed\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
