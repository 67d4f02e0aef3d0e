// Stand-alone self-test of the protocol pieces under native/ (no Python):
//   g++ -std=c++17 -O1 -I native native/tests/h2_selftest.cpp -o h2_selftest
// Exit status 0 = every check passed.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "h2.h"
#include "hpack.h"
#include "pbwire.h"

using namespace kxdp;

static int g_fail = 0;
static int g_checks = 0;

#define CHECK(cond)                                                         \
    do {                                                                    \
        g_checks++;                                                         \
        if (!(cond)) {                                                      \
            g_fail++;                                                       \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__,    \
                         #cond);                                            \
        }                                                                   \
    } while (0)

static std::string unhex(const char* s) {
    std::string out;
    int hi = -1;
    for (; *s; s++) {
        int v;
        if (*s >= '0' && *s <= '9') v = *s - '0';
        else if (*s >= 'a' && *s <= 'f') v = *s - 'a' + 10;
        else continue;
        if (hi < 0) hi = v;
        else { out.push_back((char)(hi * 16 + v)); hi = -1; }
    }
    return out;
}

static bool decode(hpack::Decoder& d, const std::string& block,
                   std::vector<hpack::Header>& out) {
    out.clear();
    return d.decode((const uint8_t*)block.data(), block.size(), out);
}

static bool has(const std::vector<hpack::Header>& hs, size_t i,
                const char* name, const char* value) {
    return i < hs.size() && hs[i].name == name && hs[i].value == value;
}

// ---------------------------------------------------------------------------
static void test_huffman() {
    CHECK(hpack::huffman().kraft_exact);
    struct { const char* text; const char* hex; } vec[] = {
        {"www.example.com", "f1e3 c2e5 f23a 6ba0 ab90 f4ff"},
        {"no-cache", "a8eb 1064 9cbf"},
        {"custom-key", "25a8 49e9 5ba9 7d7f"},
        {"custom-value", "25a8 49e9 5bb8 e8b4 bf"},
    };
    for (auto& v : vec) {
        std::string enc, dec;
        hpack::huff_encode(v.text, enc);
        CHECK(enc == unhex(v.hex));
        CHECK(hpack::huff_decode((const uint8_t*)enc.data(), enc.size(), dec));
        CHECK(dec == v.text);
    }
    // every byte value round-trips
    std::string all, enc, dec;
    for (int i = 0; i < 256; i++) all.push_back((char)i);
    hpack::huff_encode(all, enc);
    CHECK(hpack::huff_decode((const uint8_t*)enc.data(), enc.size(), dec));
    CHECK(dec == all);
    // padding rules: a whole byte of padding, zero padding, EOS in the string
    std::string bad = unhex("a8eb 1064 9cbf ff");
    dec.clear();
    CHECK(!hpack::huff_decode((const uint8_t*)bad.data(), bad.size(), dec));
    bad = unhex("a8eb 1064 9cbe");
    dec.clear();
    CHECK(!hpack::huff_decode((const uint8_t*)bad.data(), bad.size(), dec));
    bad = unhex("ffff ffff");   // 30 ones = EOS
    dec.clear();
    CHECK(!hpack::huff_decode((const uint8_t*)bad.data(), bad.size(), dec));
}

static void test_hpack_requests(bool huffman) {
    // RFC 7541 C.3 (raw) / C.4 (Huffman): three requests on one connection.
    hpack::Decoder d;
    std::vector<hpack::Header> hs;
    CHECK(decode(d, unhex(huffman
        ? "8286 8441 8cf1 e3c2 e5f2 3a6b a0ab 90f4 ff"
        : "8286 8441 0f77 7777 2e65 7861 6d70 6c65 2e63 6f6d"), hs));
    CHECK(hs.size() == 4);
    CHECK(has(hs, 0, ":method", "GET"));
    CHECK(has(hs, 1, ":scheme", "http"));
    CHECK(has(hs, 2, ":path", "/"));
    CHECK(has(hs, 3, ":authority", "www.example.com"));
    CHECK(d.dynamic_count() == 1 && d.dynamic_size() == 57);

    CHECK(decode(d, unhex(huffman
        ? "8286 84be 5886 a8eb 1064 9cbf"
        : "8286 84be 5808 6e6f 2d63 6163 6865"), hs));
    CHECK(hs.size() == 5);
    CHECK(has(hs, 3, ":authority", "www.example.com"));
    CHECK(has(hs, 4, "cache-control", "no-cache"));
    CHECK(d.dynamic_count() == 2 && d.dynamic_size() == 110);

    CHECK(decode(d, unhex(huffman
        ? "8287 85bf 4088 25a8 49e9 5ba9 7d7f 8925 a849 e95b b8e8 b4bf"
        : "8287 85bf 400a 6375 7374 6f6d 2d6b 6579 0c63 7573 746f 6d2d 7661 "
          "6c75 65"), hs));
    CHECK(hs.size() == 5);
    CHECK(has(hs, 1, ":scheme", "https"));
    CHECK(has(hs, 2, ":path", "/index.html"));
    CHECK(has(hs, 3, ":authority", "www.example.com"));
    CHECK(has(hs, 4, "custom-key", "custom-value"));
    CHECK(d.dynamic_count() == 3 && d.dynamic_size() == 164);
    CHECK(d.dynamic_at(0).name == "custom-key");
    CHECK(d.dynamic_at(2).name == ":authority");
}

static void test_hpack_eviction() {
    // RFC 7541 C.5: responses with a 256-byte table force evictions.
    hpack::Decoder d(256);
    std::vector<hpack::Header> hs;
    CHECK(decode(d, unhex(
        "4803 3330 3258 0770 7269 7661 7465 611d 4d6f 6e2c 2032 3120 4f63 "
        "7420 3230 3133 2032 303a 3133 3a32 3120 474d 546e 1768 7474 7073 "
        "3a2f 2f77 7777 2e65 7861 6d70 6c65 2e63 6f6d"), hs));
    CHECK(hs.size() == 4);
    CHECK(has(hs, 0, ":status", "302"));
    CHECK(has(hs, 1, "cache-control", "private"));
    CHECK(has(hs, 2, "date", "Mon, 21 Oct 2013 20:13:21 GMT"));
    CHECK(has(hs, 3, "location", "https://www.example.com"));
    CHECK(d.dynamic_count() == 4 && d.dynamic_size() == 222);

    CHECK(decode(d, unhex("4803 3330 37c1 c0bf"), hs));
    CHECK(hs.size() == 4);
    CHECK(has(hs, 0, ":status", "307"));
    CHECK(has(hs, 1, "cache-control", "private"));
    CHECK(has(hs, 3, "location", "https://www.example.com"));
    CHECK(d.dynamic_count() == 4 && d.dynamic_size() == 222);
    CHECK(d.dynamic_at(0).value == "307");      // ":status 302" was evicted
    CHECK(d.dynamic_at(3).name == "cache-control");

    CHECK(decode(d, unhex(
        "88c1 611d 4d6f 6e2c 2032 3120 4f63 7420 3230 3133 2032 303a 3133 "
        "3a32 3220 474d 54c0 5a04 677a 6970 7738 666f 6f3d 4153 444a 4b48 "
        "514b 425a 584f 5157 454f 5049 5541 5851 5745 4f49 553b 206d 6178 "
        "2d61 6765 3d33 3630 303b 2076 6572 7369 6f6e 3d31"), hs));
    CHECK(hs.size() == 6);
    CHECK(has(hs, 0, ":status", "200"));
    CHECK(has(hs, 2, "date", "Mon, 21 Oct 2013 20:13:22 GMT"));
    CHECK(has(hs, 4, "content-encoding", "gzip"));
    CHECK(has(hs, 5, "set-cookie",
              "foo=ASDJKHQKBZXOQWEOPIUAXQWEOIU; max-age=3600; version=1"));
    CHECK(d.dynamic_count() == 3 && d.dynamic_size() == 215);

    // size updates: shrink to 0 empties the table; growth back is allowed up
    // to the advertised limit; beyond it, or after a field, is an error.
    CHECK(decode(d, unhex("20"), hs));
    CHECK(d.dynamic_count() == 0 && d.dynamic_size() == 0 && d.max_size() == 0);
    CHECK(decode(d, unhex("3fe1 01 88"), hs));   // 31 + 225 = 256
    CHECK(d.max_size() == 256 && has(hs, 0, ":status", "200"));
    CHECK(!decode(d, unhex("3fe2 01"), hs));     // 257 > limit
    hpack::Decoder d2(256);
    CHECK(!decode(d2, unhex("88 20"), hs));      // update after a field
    // an entry larger than the table empties it and is not stored
    hpack::Decoder d3(40);
    CHECK(decode(d3, unhex("4003 6162 6301 78"), hs));   // abc: x  (36 bytes)
    CHECK(d3.dynamic_count() == 1);
    CHECK(decode(d3, unhex("4003 6162 6306 787878787878"), hs));  // 41 bytes
    CHECK(d3.dynamic_count() == 0);
    // references past the table, index 0, truncated strings
    hpack::Decoder d4;
    CHECK(!decode(d4, unhex("be"), hs));
    CHECK(!decode(d4, unhex("80"), hs));
    CHECK(!decode(d4, unhex("4005 6162"), hs));
    CHECK(!decode(d4, unhex("7fff ffff ffff ffff ff"), hs));
}

// ---------------------------------------------------------------------------
// HTTP/2 connection
// ---------------------------------------------------------------------------
struct EchoApp : h2::App {
    int calls = 0;
    std::string big = std::string(100, 'L');
    void on_rpc(h2::Conn& c, uint32_t sid, const std::string& path,
                std::string& msg) override {
        calls++;
        if (path == "/t/Echo") c.reply_unary(sid, msg);
        else if (path == "/t/Watch") { c.start_stream(sid); c.push_message(sid, big); }
        else c.reply_error(sid, h2::GRPC_UNIMPLEMENTED, "no such method");
    }
};

struct Frame {
    h2::FrameHeader h;
    std::string payload;
};

static std::vector<Frame> take_frames(h2::Conn& c) {
    std::vector<Frame> fs;
    std::string& out = c.out();
    size_t off = 0;
    while (out.size() - off >= 9) {
        Frame f;
        h2::parse_frame_header((const uint8_t*)out.data() + off, f.h);
        if (out.size() - off < 9 + (size_t)f.h.length) break;
        f.payload.assign(out, off + 9, f.h.length);
        off += 9 + f.h.length;
        fs.push_back(std::move(f));
    }
    CHECK(off == out.size());
    out.clear();
    return fs;
}

static std::string frame(uint8_t type, uint8_t flags, uint32_t sid,
                         const std::string& payload) {
    std::string f;
    h2::put_frame_header(f, (uint32_t)payload.size(), type, flags, sid);
    return f + payload;
}

static std::string request_block(const char* path) {
    std::string b;
    b.push_back((char)0x83);   // :method POST
    b.push_back((char)0x86);   // :scheme http
    hpack::encode_literal(b, ":path", path);
    hpack::encode_literal(b, "content-type", "application/grpc");
    hpack::encode_literal(b, "te", "trailers");
    return b;
}

static std::string grpc_msg(const std::string& payload) {
    std::string m;
    m.push_back(0);
    h2::put_u32(m, (uint32_t)payload.size());
    return m + payload;
}

static bool feed(h2::Conn& c, const std::string& s) {
    return c.feed((const uint8_t*)s.data(), s.size());
}

static std::string preface() {
    return std::string(h2::kPreface, h2::kPrefaceLen) +
           frame(h2::SETTINGS, 0, 0, "");
}

static const Frame* find_frame(const std::vector<Frame>& fs, uint8_t type,
                               uint32_t sid) {
    for (auto& f : fs)
        if (f.h.type == type && f.h.stream == sid) return &f;
    return nullptr;
}

static void test_unary_and_frames() {
    EchoApp app;
    {   // a clean unary, delivered one byte at a time
        h2::Conn c(&app);
        std::string in = preface() +
            frame(h2::HEADERS, h2::END_HEADERS, 1, request_block("/t/Echo")) +
            frame(h2::DATA, h2::END_STREAM, 1, grpc_msg("hello"));
        for (char ch : in) CHECK(c.feed((const uint8_t*)&ch, 1));
        auto fs = take_frames(c);
        CHECK(app.calls == 1);
        const Frame* d = find_frame(fs, h2::DATA, 1);
        CHECK(d && d->payload == grpc_msg("hello"));
        CHECK(fs.back().h.type == h2::HEADERS &&
              (fs.back().h.flags & h2::END_STREAM));
        CHECK(c.open_streams() == 0);
        // truncated frame: header says 8, only 3 bytes yet → just buffered
        std::string ping = frame(h2::PING, 0, 0, "12345678");
        CHECK(feed(c, ping.substr(0, 12)));
        CHECK(c.out().empty() && c.buffered() == 12);
        CHECK(feed(c, ping.substr(12)));
        fs = take_frames(c);
        CHECK(fs.size() == 1 && fs[0].h.type == h2::PING &&
              (fs[0].h.flags & h2::ACK) && fs[0].payload == "12345678");
    }
    {   // padded + priority HEADERS split over two CONTINUATIONs
        h2::Conn c(&app);
        std::string b = request_block("/t/Echo");
        std::string first = std::string(1, (char)3) +       // pad length
                            std::string("\0\0\0\0\x10", 5) + // priority
                            b.substr(0, 4) + std::string(3, '\0');
        CHECK(feed(c, preface() +
            frame(h2::HEADERS, h2::PADDED | h2::HAS_PRIORITY, 1, first) +
            frame(h2::CONTINUATION, 0, 1, b.substr(4, 7)) +
            frame(h2::CONTINUATION, h2::END_HEADERS, 1, b.substr(11)) +
            frame(h2::DATA, h2::END_STREAM | h2::PADDED, 1,
                  std::string(1, (char)2) + grpc_msg("x") + std::string(2, '\0'))));
        auto fs = take_frames(c);
        const Frame* d = find_frame(fs, h2::DATA, 1);
        CHECK(d && d->payload == grpc_msg("x"));
    }
    {   // padding longer than the frame
        h2::Conn c(&app);
        CHECK(!feed(c, preface() + frame(h2::HEADERS, h2::PADDED | h2::END_HEADERS,
                                         1, std::string(1, (char)9) + "abc")));
        CHECK(c.goaway_code() == h2::PROTOCOL_ERROR);
    }
    {   // CONTINUATION without HEADERS
        h2::Conn c(&app);
        CHECK(!feed(c, preface() + frame(h2::CONTINUATION, h2::END_HEADERS, 1, "")));
        CHECK(c.goaway_code() == h2::PROTOCOL_ERROR);
    }
    {   // another frame between HEADERS and CONTINUATION
        h2::Conn c(&app);
        CHECK(!feed(c, preface() + frame(h2::HEADERS, 0, 1, "") +
                       frame(h2::PING, 0, 0, "12345678")));
        CHECK(c.goaway_code() == h2::PROTOCOL_ERROR);
    }
    {   // oversize frame: rejected from its header alone
        h2::Conn c(&app);
        std::string hdr;
        h2::put_frame_header(hdr, h2::kOurMaxFrame + 1, h2::DATA, 0, 1);
        CHECK(!feed(c, preface() + hdr));
        CHECK(c.goaway_code() == h2::FRAME_SIZE_ERROR && c.want_close());
        auto fs = take_frames(c);
        CHECK(fs.back().h.type == h2::GOAWAY);
    }
    {   // garbage preface
        h2::Conn c(&app);
        CHECK(!feed(c, "GET / HTTP/1.1\r\n\r\n"));
        CHECK(c.goaway_code() == h2::PROTOCOL_ERROR);
    }
    {   // bad HPACK → COMPRESSION_ERROR; PUSH_PROMISE → PROTOCOL_ERROR
        h2::Conn c(&app);
        CHECK(!feed(c, preface() + frame(h2::HEADERS, h2::END_HEADERS, 1, "\xbe")));
        CHECK(c.goaway_code() == h2::COMPRESSION_ERROR);
        h2::Conn c2(&app);
        CHECK(!feed(c2, preface() + frame(h2::PUSH_PROMISE, h2::END_HEADERS, 1, "abcd")));
        CHECK(c2.goaway_code() == h2::PROTOCOL_ERROR);
    }
    {   // compressed flag → status 12, connection stays usable
        h2::Conn c(&app);
        std::string m = grpc_msg("zz");
        m[0] = 1;
        CHECK(feed(c, preface() +
            frame(h2::HEADERS, h2::END_HEADERS, 1, request_block("/t/Echo")) +
            frame(h2::DATA, h2::END_STREAM, 1, m) +
            frame(h2::HEADERS, h2::END_HEADERS, 3, request_block("/t/Nope")) +
            frame(h2::DATA, h2::END_STREAM, 3, grpc_msg(""))));
        auto fs = take_frames(c);
        const Frame* t1 = find_frame(fs, h2::HEADERS, 1);
        const Frame* t3 = find_frame(fs, h2::HEADERS, 3);
        CHECK(t1 && t1->payload.find("grpc-status\x02" "12") != std::string::npos);
        CHECK(t3 && t3->payload.find("grpc-status\x02" "12") != std::string::npos);
        CHECK(!c.dead());
    }
}

static void test_flow_control() {
    EchoApp app;
    h2::Conn c(&app);
    // INITIAL_WINDOW_SIZE = 16: the 105-byte stream message comes in pieces
    std::string settings("\x00\x04\x00\x00\x00\x10", 6);
    CHECK(feed(c, std::string(h2::kPreface, h2::kPrefaceLen) +
        frame(h2::SETTINGS, 0, 0, settings) +
        frame(h2::HEADERS, h2::END_HEADERS, 1, request_block("/t/Watch")) +
        frame(h2::DATA, h2::END_STREAM, 1, grpc_msg(""))));
    std::string got;
    auto collect = [&](const std::vector<Frame>& fs) {
        size_t n = 0;
        for (auto& f : fs)
            if (f.h.type == h2::DATA) { got += f.payload; n += f.payload.size(); }
        return n;
    };
    CHECK(collect(take_frames(c)) == 16);
    c.push_message(1, "old");      // blocked: queued behind the first
    c.push_message(1, "newest");   // replaces "old"
    CHECK(c.out().empty());
    int rounds = 0;
    while (got.size() < 105 + 11 && rounds++ < 100) {
        std::string inc;
        h2::put_u32(inc, 16);
        CHECK(feed(c, frame(h2::WINDOW_UPDATE, 0, 1, inc)));
        CHECK(collect(take_frames(c)) <= 16);
    }
    CHECK(got == grpc_msg(app.big) + grpc_msg("newest"));
    // raising INITIAL_WINDOW_SIZE applies the delta to the open stream
    // (8 grants of 16 carried 116 bytes: 12 bytes of window are left)
    c.push_message(1, std::string(40, 'q'));
    CHECK(collect(take_frames(c)) == 12);
    std::string bigger("\x00\x04\x00\x00\x00\x40", 6);   // 16 → 64
    CHECK(feed(c, frame(h2::SETTINGS, 0, 0, bigger)));
    CHECK(collect(take_frames(c)) == 45 - 12);
    // window overflow is a connection error
    std::string inc;
    h2::put_u32(inc, 0x7fffffff);
    CHECK(!feed(c, frame(h2::WINDOW_UPDATE, 0, 0, inc)));
    CHECK(c.goaway_code() == h2::FLOW_CONTROL_ERROR);

    // receive side: > 65535 request bytes on one connection keep flowing
    h2::Conn r(&app);
    CHECK(feed(r, preface()));
    take_frames(r);
    size_t updates = 0;
    for (uint32_t sid = 1; sid < 2 * 3000; sid += 2) {
        CHECK(feed(r, frame(h2::HEADERS, h2::END_HEADERS, sid, request_block("/t/Echo")) +
                      frame(h2::DATA, h2::END_STREAM, sid, grpc_msg(std::string(25, 'r')))));
        for (auto& f : take_frames(r))
            if (f.h.type == h2::WINDOW_UPDATE && f.h.stream == 0) updates++;
    }
    CHECK(!r.dead() && updates >= 5);
    // shutdown: GOAWAY + OK trailers on the watch stream
    h2::Conn s(&app);
    CHECK(feed(s, preface() +
        frame(h2::HEADERS, h2::END_HEADERS, 1, request_block("/t/Watch")) +
        frame(h2::DATA, h2::END_STREAM, 1, grpc_msg(""))));
    take_frames(s);
    s.begin_shutdown();
    auto fs = take_frames(s);
    CHECK(find_frame(fs, h2::GOAWAY, 0));
    const Frame* t = find_frame(fs, h2::HEADERS, 1);
    CHECK(t && (t->h.flags & h2::END_STREAM) &&
          t->payload.find("grpc-status\x01" "0") != std::string::npos);
    CHECK(s.want_close());
}

static void test_pbwire() {
    std::string creq, req;
    pb::put_bytes(creq, 1, "70");
    pb::put_bytes(creq, 1, "71");
    pb::put_bytes(req, 1, creq);
    pb::put_bytes(req, 1, "");
    pb::put_varint(req, (9 << 3) | 0);   // unknown varint field
    pb::put_varint(req, 300);
    std::vector<std::vector<std::string>> out;
    CHECK(pb::parse_allocate_request(req, out));
    CHECK(out.size() == 2 && out[0].size() == 2 && out[0][1] == "71" &&
          out[1].empty());
    out.clear();
    CHECK(!pb::parse_allocate_request(req.substr(0, 5), out));
    out.clear();
    CHECK(!pb::parse_allocate_request(std::string("\x0a\xff\xff\xff\xff\x0f", 6), out));
}

// Pseudo-random input against the state machine: must not crash, hang, or
// hold more than a frame of input / a bounded amount of output.
static void test_fuzz() {
    EchoApp app;
    uint64_t x = 0x9e3779b97f4a7c15ull;
    auto rnd = [&]() {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        return x;
    };
    std::string block = request_block("/t/Echo");
    size_t max_out = 0, max_in = 0;
    for (int iter = 0; iter < 4000; iter++) {
        h2::Conn c(&app);
        std::string in;
        if (iter % 4) in = preface();
        int n = 1 + (int)(rnd() % 24);
        uint32_t sid = 1;
        for (int i = 0; i < n; i++) {
            uint64_t r = rnd();
            switch (r % 8) {
            case 0: {   // raw noise
                size_t len = (r >> 8) % 40;
                for (size_t k = 0; k < len; k++) in.push_back((char)rnd());
                break;
            }
            case 1: case 2: {   // well-formed header, random payload
                size_t len = (r >> 8) % 64;
                std::string p;
                for (size_t k = 0; k < len; k++) p.push_back((char)rnd());
                in += frame((uint8_t)((r >> 16) % 11), (uint8_t)(r >> 24),
                            (uint32_t)((r >> 32) % 8), p);
                break;
            }
            case 3:
                in += frame(h2::HEADERS, h2::END_HEADERS | ((r >> 8) & 1), sid, block);
                break;
            case 4:
                in += frame(h2::DATA, (r >> 8) & 1, sid,
                            grpc_msg(std::string((r >> 16) % 50, 'd')));
                break;
            case 5: sid += 2; break;
            case 6: {
                std::string v;
                h2::put_u32(v, (uint32_t)rnd());
                in += frame(h2::WINDOW_UPDATE, 0, (r >> 8) & 1 ? sid : 0, v);
                break;
            }
            default: {
                std::string s;
                s.push_back(0); s.push_back((char)(1 + (r >> 8) % 6));
                h2::put_u32(s, (uint32_t)rnd() >> ((r >> 16) % 32));
                in += frame(h2::SETTINGS, 0, 0, s);
            }
            }
        }
        size_t off = 0;
        while (off < in.size()) {
            size_t chunk = 1 + rnd() % 97;
            chunk = std::min(chunk, in.size() - off);
            bool alive = c.feed((const uint8_t*)in.data() + off, chunk);
            off += chunk;
            max_in = std::max(max_in, c.buffered());
            max_out = std::max(max_out, c.out().size());
            if (!alive) { CHECK(c.want_close()); break; }
        }
        CHECK(c.open_streams() <= h2::kMaxStreams);
    }
    CHECK(max_in <= 9 + h2::kOurMaxFrame);
    CHECK(max_out <= 64 * 1024);
}

int main() {
    test_huffman();
    test_hpack_requests(false);
    test_hpack_requests(true);
    test_hpack_eviction();
    test_unary_and_frames();
    test_flow_control();
    test_pbwire();
    test_fuzz();
    std::printf("h2_selftest: %d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
