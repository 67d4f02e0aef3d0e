// HPACK (RFC 7541) for the native gRPC server: full decoder (static and
// dynamic table, size updates, all literal forms, Huffman) and a trivial
// encoder (literal-without-indexing, no Huffman — always valid, and it
// means the peer's HEADER_TABLE_SIZE never matters to us).
//
// No pybind11 / Python.h here: native/tests/h2_selftest.cpp exercises this
// file stand-alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <deque>
#include <string>
#include <utility>
#include <vector>

namespace kxdp {
namespace hpack {

// ---------------------------------------------------------------------------
// Huffman. The HPACK code (RFC 7541 Appendix B) is canonical: within one
// code length, codes are consecutive in symbol order, and the first code of
// a length follows the last code of the shorter length shifted left. So the
// 257 lengths below determine every code.
// ---------------------------------------------------------------------------
static const uint8_t kHuffLen[257] = {
    // 0..31
    13, 23, 28, 28, 28, 28, 28, 28, 28, 24, 30, 28, 28, 30, 28, 28,
    28, 28, 28, 28, 28, 28, 30, 28, 28, 28, 28, 28, 28, 28, 28, 28,
    // ' ' ! " # $ % & ' ( ) * + , - . /
    6, 10, 10, 12, 13, 6, 8, 11, 10, 10, 8, 11, 8, 6, 6, 6,
    // 0..9 : ; < = > ?
    5, 5, 5, 6, 6, 6, 6, 6, 6, 6, 7, 8, 15, 6, 12, 10,
    // @ A..O
    13, 6, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7, 7,
    // P..Z [ \ ] ^ _
    7, 7, 7, 7, 7, 7, 7, 7, 8, 7, 8, 13, 19, 13, 14, 6,
    // ` a..o
    15, 5, 6, 5, 6, 5, 6, 6, 6, 5, 7, 7, 6, 6, 6, 5,
    // p..z { | } ~ DEL
    6, 7, 6, 5, 5, 6, 7, 7, 7, 7, 7, 15, 11, 14, 13, 28,
    // 128..143
    20, 22, 20, 20, 22, 22, 22, 23, 22, 23, 23, 23, 23, 23, 24, 23,
    // 144..159
    24, 24, 22, 23, 24, 23, 23, 23, 23, 21, 22, 23, 22, 23, 23, 24,
    // 160..175
    22, 21, 20, 22, 22, 23, 23, 21, 23, 22, 22, 24, 21, 22, 23, 23,
    // 176..191
    21, 21, 22, 21, 23, 22, 23, 23, 20, 22, 22, 22, 23, 22, 22, 23,
    // 192..207
    26, 26, 20, 19, 22, 23, 22, 25, 26, 26, 26, 27, 27, 26, 24, 25,
    // 208..223
    19, 21, 26, 27, 27, 26, 27, 24, 21, 21, 26, 26, 28, 27, 27, 27,
    // 224..239
    20, 24, 20, 21, 22, 21, 21, 23, 22, 22, 25, 25, 24, 24, 26, 23,
    // 240..255
    26, 27, 26, 26, 27, 27, 27, 27, 27, 28, 27, 27, 27, 27, 27, 26,
    // EOS
    30,
};

struct Huffman {
    uint32_t code[257];          // right-aligned code per symbol
    uint32_t first_code[32];     // first code of each length
    uint16_t first_index[32];    // index into sorted[] of that code
    uint16_t count[32];          // symbols of each length
    uint16_t sorted[257];        // symbols ordered by (length, value)
    bool kraft_exact = false;    // sum 2^-len == 1

    Huffman() {
        for (int l = 0; l < 32; l++) count[l] = 0;
        for (int s = 0; s < 257; s++) count[kHuffLen[s]]++;
        uint64_t kraft = 0;      // in units of 2^-30
        uint32_t c = 0;
        uint16_t idx = 0;
        for (int l = 1; l <= 30; l++) {
            c <<= 1;
            first_code[l] = c;
            first_index[l] = idx;
            for (int s = 0; s < 257; s++) {
                if (kHuffLen[s] != l) continue;
                code[s] = c++;
                sorted[idx++] = (uint16_t)s;
                kraft += 1ull << (30 - l);
            }
        }
        first_code[0] = first_code[31] = 0;
        first_index[0] = first_index[31] = 0;
        kraft_exact = kraft == (1ull << 30);
    }
};

inline const Huffman& huffman() {
    static const Huffman h;
    return h;
}

inline void huff_encode(const std::string& in, std::string& out) {
    const Huffman& h = huffman();
    uint64_t acc = 0;
    int bits = 0;
    for (unsigned char ch : in) {
        acc = (acc << kHuffLen[ch]) | h.code[ch];
        bits += kHuffLen[ch];
        while (bits >= 8) {
            out.push_back((char)((acc >> (bits - 8)) & 0xff));
            bits -= 8;
        }
    }
    if (bits) {   // pad with the most significant bits of EOS (all ones)
        out.push_back((char)(((acc << (8 - bits)) | (0xffu >> bits)) & 0xff));
    }
}

// False on EOS inside the string, padding longer than 7 bits, or padding
// that is not all ones (RFC 7541 §5.2).
inline bool huff_decode(const uint8_t* p, size_t n, std::string& out) {
    const Huffman& h = huffman();
    uint32_t cur = 0;
    int len = 0;
    bool all_ones = true;
    for (size_t i = 0; i < n; i++) {
        for (int b = 7; b >= 0; b--) {
            uint32_t bit = (p[i] >> b) & 1;
            cur = (cur << 1) | bit;
            all_ones = all_ones && bit;
            len++;
            if (len > 30) return false;
            uint32_t off = cur - h.first_code[len];
            if (cur >= h.first_code[len] && off < h.count[len]) {
                uint16_t sym = h.sorted[h.first_index[len] + off];
                if (sym == 256) return false;
                out.push_back((char)sym);
                cur = 0;
                len = 0;
                all_ones = true;
            }
        }
    }
    return len < 8 && all_ones;
}

// ---------------------------------------------------------------------------
// Tables
// ---------------------------------------------------------------------------
struct Header {
    std::string name, value;
};

static const char* const kStatic[61][2] = {
    {":authority", ""}, {":method", "GET"}, {":method", "POST"},
    {":path", "/"}, {":path", "/index.html"}, {":scheme", "http"},
    {":scheme", "https"}, {":status", "200"}, {":status", "204"},
    {":status", "206"}, {":status", "304"}, {":status", "400"},
    {":status", "404"}, {":status", "500"}, {"accept-charset", ""},
    {"accept-encoding", "gzip, deflate"}, {"accept-language", ""},
    {"accept-ranges", ""}, {"accept", ""},
    {"access-control-allow-origin", ""}, {"age", ""}, {"allow", ""},
    {"authorization", ""}, {"cache-control", ""},
    {"content-disposition", ""}, {"content-encoding", ""},
    {"content-language", ""}, {"content-length", ""},
    {"content-location", ""}, {"content-range", ""}, {"content-type", ""},
    {"cookie", ""}, {"date", ""}, {"etag", ""}, {"expect", ""},
    {"expires", ""}, {"from", ""}, {"host", ""}, {"if-match", ""},
    {"if-modified-since", ""}, {"if-none-match", ""}, {"if-range", ""},
    {"if-unmodified-since", ""}, {"last-modified", ""}, {"link", ""},
    {"location", ""}, {"max-forwards", ""}, {"proxy-authenticate", ""},
    {"proxy-authorization", ""}, {"range", ""}, {"referer", ""},
    {"refresh", ""}, {"retry-after", ""}, {"server", ""},
    {"set-cookie", ""}, {"strict-transport-security", ""},
    {"transfer-encoding", ""}, {"user-agent", ""}, {"vary", ""},
    {"via", ""}, {"www-authenticate", ""},
};

class Decoder {
public:
    // `limit` is the SETTINGS_HEADER_TABLE_SIZE we advertise (we never send
    // one, so the protocol default of 4096 holds).
    explicit Decoder(size_t limit = 4096) : limit_(limit), max_(limit) {}

    // Decode one complete header block. False = COMPRESSION_ERROR.
    // `max_list` bounds the decoded size (names + values + 32 each).
    bool decode(const uint8_t* p, size_t n, std::vector<Header>& out,
                size_t max_list = 65536) {
        const uint8_t* end = p + n;
        bool seen_field = false;
        size_t list = 0;
        while (p < end) {
            uint8_t b = *p;
            Header h;
            if (b & 0x80) {                       // indexed
                uint64_t idx;
                if (!read_int(p, end, 7, idx) || !lookup(idx, h)) return false;
            } else if ((b & 0xe0) == 0x20) {      // dynamic table size update
                uint64_t sz;
                if (seen_field) return false;     // only at block start
                if (!read_int(p, end, 5, sz) || sz > limit_) return false;
                max_ = (size_t)sz;
                evict();
                continue;
            } else {
                bool incremental = (b & 0xc0) == 0x40;
                int prefix = incremental ? 6 : 4;  // 0000 / 0001 share 4 bits
                uint64_t idx;
                if (!read_int(p, end, prefix, idx)) return false;
                if (idx) {
                    Header nm;
                    if (!lookup(idx, nm)) return false;
                    h.name = std::move(nm.name);
                } else if (!read_string(p, end, h.name)) {
                    return false;
                }
                if (!read_string(p, end, h.value)) return false;
                if (incremental) insert(h);
            }
            seen_field = true;
            list += h.name.size() + h.value.size() + 32;
            if (list > max_list) return false;
            out.push_back(std::move(h));
        }
        return true;
    }

    size_t dynamic_size() const { return size_; }
    size_t dynamic_count() const { return dyn_.size(); }
    size_t max_size() const { return max_; }
    const Header& dynamic_at(size_t i) const { return dyn_[i]; }  // 0 = newest

private:
    static bool read_int(const uint8_t*& p, const uint8_t* end, int prefix,
                         uint64_t& v) {
        if (p >= end) return false;
        const uint32_t mask = (1u << prefix) - 1;
        v = *p++ & mask;
        if (v < mask) return true;
        int shift = 0;
        while (true) {
            if (p >= end || shift > 28) return false;   // < 2^35, ample
            uint8_t b = *p++;
            v += (uint64_t)(b & 0x7f) << shift;
            shift += 7;
            if (!(b & 0x80)) return true;
        }
    }

    static bool read_string(const uint8_t*& p, const uint8_t* end,
                            std::string& out) {
        if (p >= end) return false;
        bool huff = *p & 0x80;
        uint64_t len;
        if (!read_int(p, end, 7, len)) return false;
        if (len > (uint64_t)(end - p)) return false;
        if (huff) {
            if (!huff_decode(p, (size_t)len, out)) return false;
        } else {
            out.assign((const char*)p, (size_t)len);
        }
        p += len;
        return true;
    }

    bool lookup(uint64_t idx, Header& h) const {
        if (idx == 0) return false;
        if (idx <= 61) {
            h.name = kStatic[idx - 1][0];
            h.value = kStatic[idx - 1][1];
            return true;
        }
        idx -= 62;
        if (idx >= dyn_.size()) return false;
        h = dyn_[(size_t)idx];
        return true;
    }

    void insert(const Header& h) {
        size_t sz = h.name.size() + h.value.size() + 32;
        if (sz > max_) {          // larger than the table: empties it
            dyn_.clear();
            size_ = 0;
            return;
        }
        dyn_.push_front(h);
        size_ += sz;
        evict();
    }

    void evict() {
        while (size_ > max_ && !dyn_.empty()) {
            size_ -= dyn_.back().name.size() + dyn_.back().value.size() + 32;
            dyn_.pop_back();
        }
    }

    std::deque<Header> dyn_;
    size_t size_ = 0;
    size_t limit_;
    size_t max_;
};

// ---------------------------------------------------------------------------
// Encoder: literal header field without indexing, new name, raw strings.
// ---------------------------------------------------------------------------
inline void put_int(std::string& out, uint8_t first, int prefix, uint64_t v) {
    const uint32_t mask = (1u << prefix) - 1;
    if (v < mask) {
        out.push_back((char)(first | v));
        return;
    }
    out.push_back((char)(first | mask));
    v -= mask;
    while (v >= 128) {
        out.push_back((char)((v & 0x7f) | 0x80));
        v >>= 7;
    }
    out.push_back((char)v);
}

inline void encode_literal(std::string& out, const std::string& name,
                           const std::string& value) {
    out.push_back(0x00);
    put_int(out, 0x00, 7, name.size());
    out += name;
    put_int(out, 0x00, 7, value.size());
    out += value;
}

}  // namespace hpack
}  // namespace kxdp
