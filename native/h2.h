// HTTP/2 (RFC 7540) server-side connection state machine carrying gRPC.
//
// Conn is IO-free: feed() takes whatever bytes arrived, appends whatever
// must be written to out(), and hands every complete request to the App.
// The epoll loop in xpu_grpc_server.cpp owns the sockets; the stand-alone
// native/tests/h2_selftest.cpp drives the same class with byte strings.
// No pybind11 / Python.h here.
//
// Every RPC of the services we carry takes exactly one request message, so
// a request is dispatched when the client half-closes (END_STREAM) with one
// complete length-prefixed message. The App answers synchronously with
// reply_unary(), reply_error(), or start_stream() (server streaming).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "hpack.h"

namespace kxdp {
namespace h2 {

enum FrameType : uint8_t {
    DATA = 0, HEADERS = 1, PRIORITY = 2, RST_STREAM = 3, SETTINGS = 4,
    PUSH_PROMISE = 5, PING = 6, GOAWAY = 7, WINDOW_UPDATE = 8,
    CONTINUATION = 9,
};

enum Flag : uint8_t {
    END_STREAM = 0x1, ACK = 0x1, END_HEADERS = 0x4, PADDED = 0x8,
    HAS_PRIORITY = 0x20,
};

enum ErrorCode : uint32_t {
    NO_ERROR = 0, PROTOCOL_ERROR = 1, INTERNAL_ERROR = 2,
    FLOW_CONTROL_ERROR = 3, STREAM_CLOSED = 5, FRAME_SIZE_ERROR = 6,
    REFUSED_STREAM = 7, CANCEL = 8, COMPRESSION_ERROR = 9,
    ENHANCE_YOUR_CALM = 0xb,
};

// gRPC status codes used here
enum GrpcStatus : int {
    GRPC_OK = 0, GRPC_UNKNOWN = 2, GRPC_INVALID_ARGUMENT = 3,
    GRPC_RESOURCE_EXHAUSTED = 8, GRPC_UNIMPLEMENTED = 12, GRPC_INTERNAL = 13,
    GRPC_UNAVAILABLE = 14,
};

static const char kPreface[] = "PRI * HTTP/2.0\r\n\r\nSM\r\n\r\n";
constexpr size_t kPrefaceLen = 24;
constexpr uint32_t kOurMaxFrame = 16384;        // what we advertise (default)
constexpr int64_t kDefaultWindow = 65535;
constexpr int64_t kMaxWindow = 0x7fffffff;
constexpr uint32_t kMaxStreams = 64;            // MAX_CONCURRENT_STREAMS
constexpr size_t kMaxHeaderBlock = 65536;
constexpr size_t kMaxMessage = 4u << 20;        // gRPC's default receive cap
constexpr size_t kMaxOutBuffer = 8u << 20;      // peer stopped reading
constexpr uint32_t kWindowSlack = 16384;        // replenish after this much

struct FrameHeader {
    uint32_t length;
    uint8_t type, flags;
    uint32_t stream;
};

inline void parse_frame_header(const uint8_t* p, FrameHeader& h) {
    h.length = ((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 8) | p[2];
    h.type = p[3];
    h.flags = p[4];
    h.stream = (((uint32_t)p[5] << 24) | ((uint32_t)p[6] << 16) |
                ((uint32_t)p[7] << 8) | p[8]) & 0x7fffffffu;
}

inline void put_frame_header(std::string& out, uint32_t len, uint8_t type,
                             uint8_t flags, uint32_t stream) {
    const char h[9] = {
        (char)(len >> 16), (char)(len >> 8), (char)len, (char)type,
        (char)flags, (char)(stream >> 24), (char)(stream >> 16),
        (char)(stream >> 8), (char)stream,
    };
    out.append(h, 9);
}

inline void put_u32(std::string& out, uint32_t v) {
    const char b[4] = {(char)(v >> 24), (char)(v >> 16), (char)(v >> 8), (char)v};
    out.append(b, 4);
}

inline uint32_t get_u32(const uint8_t* p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) |
           ((uint32_t)p[2] << 8) | p[3];
}

// Remove the Pad Length octet + padding (PADDED) and the 5 priority octets
// (HEADERS with PRIORITY) from a DATA/HEADERS payload. False = malformed.
inline bool strip_padding(uint8_t type, uint8_t flags, const uint8_t*& p,
                          size_t& n) {
    if (flags & PADDED) {
        if (n < 1) return false;
        size_t pad = p[0];
        p++;
        n--;
        if (pad > n) return false;
        n -= pad;
    }
    if (type == HEADERS && (flags & HAS_PRIORITY)) {
        if (n < 5) return false;
        p += 5;
        n -= 5;
    }
    return true;
}

// grpc-message is percent-encoded (gRPC over HTTP/2 spec, Status-Message).
inline std::string percent_encode(const std::string& s) {
    static const char* hex = "0123456789ABCDEF";
    std::string out;
    for (unsigned char c : s) {
        if (c >= 0x20 && c <= 0x7e && c != '%') {
            out.push_back((char)c);
        } else {
            out.push_back('%');
            out.push_back(hex[c >> 4]);
            out.push_back(hex[c & 15]);
        }
    }
    return out;
}

class Conn;

struct App {
    virtual ~App() {}
    // One complete request. `msg` is the message without the gRPC prefix
    // and may be consumed. Must answer before returning.
    virtual void on_rpc(Conn& c, uint32_t sid, const std::string& path,
                        std::string& msg) = 0;
};

struct Stream {
    std::string path;
    std::string body;            // request bytes incl. 5-byte prefix
    bool remote_closed = false;
    bool headers_sent = false;
    bool watch = false;          // server-streaming subscriber
    int64_t send_window = 0;
    int64_t recv_window = kDefaultWindow;
    uint32_t recv_unacked = 0;
    std::string pending;         // framed message bytes being sent
    size_t pending_off = 0;
    std::string next_msg;        // newest whole message behind `pending`
    bool has_next = false;
    std::string trailers;        // header block to end the stream with
    bool has_trailers = false;
};

class Conn {
public:
    explicit Conn(App* app) : app_(app) {
        // server preface: SETTINGS{MAX_CONCURRENT_STREAMS}
        put_frame_header(out_, 6, SETTINGS, 0, 0);
        out_.push_back(0);
        out_.push_back(3);
        put_u32(out_, kMaxStreams);
    }

    std::string& out() { return out_; }
    // true once the connection must be closed after out() is flushed
    bool want_close() const {
        return dead_ || ((peer_goaway_ || shutting_down_) && streams_.empty());
    }
    bool dead() const { return dead_; }
    size_t open_streams() const { return streams_.size(); }
    size_t watch_streams() const { return watch_streams_; }   // open server streams
    size_t buffered() const { return in_.size(); }
    uint32_t goaway_code() const { return goaway_code_; }

    // Consume bytes from the peer. Returns false once the connection is
    // dead (a GOAWAY may be waiting in out()).
    bool feed(const uint8_t* data, size_t n) {
        if (dead_) return false;
        const uint8_t* p = data;
        size_t len = n;
        if (!in_.empty()) {
            in_.append((const char*)data, n);
            p = (const uint8_t*)in_.data();
            len = in_.size();
        }
        size_t off = 0;
        while (!dead_ && off < len) {
            if (!preface_done_) {
                size_t want = kPrefaceLen - preface_seen_;
                size_t take = std::min(want, len - off);
                if (std::memcmp(p + off, kPreface + preface_seen_, take) != 0) {
                    conn_error(PROTOCOL_ERROR);
                    break;
                }
                preface_seen_ += take;
                off += take;
                preface_done_ = preface_seen_ == kPrefaceLen;
                continue;
            }
            if (len - off < 9) break;
            FrameHeader h;
            parse_frame_header(p + off, h);
            if (h.length > kOurMaxFrame) {
                conn_error(FRAME_SIZE_ERROR);
                break;
            }
            if (len - off < 9 + (size_t)h.length) break;
            on_frame(h, p + off + 9);
            off += 9 + h.length;
            if (out_.size() > kMaxOutBuffer) dead_ = true;
        }
        if (dead_) {
            in_.clear();
            return false;
        }
        if (off == len) {
            in_.clear();
        } else if (in_.empty()) {
            in_.assign((const char*)p + off, len - off);
        } else {
            in_.erase(0, off);
        }
        return true;
    }

    // ---- answers (called by the App) ----------------------------------
    void reply_unary(uint32_t sid, const std::string& payload) {
        Stream* s = find(sid);
        if (!s) return;
        send_response_headers(sid, *s);
        frame_message(payload, s->pending);
        s->pending_off = 0;
        s->trailers = ok_trailers();
        s->has_trailers = true;
        flush_stream(sid);
    }

    void reply_error(uint32_t sid, int status, const std::string& message) {
        Stream* s = find(sid);
        if (!s) return;
        std::string block;
        if (!s->headers_sent) {   // Trailers-Only
            hpack::encode_literal(block, ":status", "200");
            hpack::encode_literal(block, "content-type", "application/grpc");
        }
        hpack::encode_literal(block, "grpc-status", std::to_string(status));
        if (!message.empty())
            hpack::encode_literal(block, "grpc-message", percent_encode(message));
        s->pending.clear();
        s->pending_off = 0;
        s->has_next = false;
        send_header_block(sid, block, true);
        close_local(sid);
    }

    void start_stream(uint32_t sid) {
        Stream* s = find(sid);
        if (!s) return;
        send_response_headers(sid, *s);
        if (!s->watch) watch_streams_++;
        s->watch = true;
    }

    // Queue a message on a server stream. While the stream is blocked on
    // flow control only the newest queued message is kept.
    void push_message(uint32_t sid, const std::string& payload) {
        Stream* s = find(sid);
        if (!s || s->has_trailers) return;
        if (s->pending.empty()) {
            frame_message(payload, s->pending);
            s->pending_off = 0;
            flush_stream(sid);
        } else {
            s->next_msg.clear();
            frame_message(payload, s->next_msg);
            s->has_next = true;
        }
    }

    void broadcast(const std::string& payload) {
        std::vector<uint32_t> ids;
        for (auto& kv : streams_)
            if (kv.second.watch) ids.push_back(kv.first);
        for (uint32_t sid : ids) push_message(sid, payload);
    }

    void finish_stream(uint32_t sid, int status) {
        Stream* s = find(sid);
        if (!s || s->has_trailers) return;
        if (s->watch) watch_streams_--;
        s->watch = false;
        s->trailers.clear();
        hpack::encode_literal(s->trailers, "grpc-status", std::to_string(status));
        s->has_trailers = true;
        flush_stream(sid);
    }

    // Orderly server shutdown: GOAWAY, end server streams with OK.
    void begin_shutdown() {
        if (dead_ || shutting_down_) return;
        shutting_down_ = true;
        send_goaway(NO_ERROR);
        end_watch_streams(GRPC_OK);
    }

private:
    Stream* find(uint32_t sid) {
        auto it = streams_.find(sid);
        return it == streams_.end() ? nullptr : &it->second;
    }

    void erase_stream(uint32_t sid) {
        auto it = streams_.find(sid);
        if (it == streams_.end()) return;
        if (it->second.watch) watch_streams_--;
        streams_.erase(it);
    }

    static void frame_message(const std::string& payload, std::string& out) {
        out.push_back(0);
        put_u32(out, (uint32_t)payload.size());
        out += payload;
    }

    static const std::string& response_headers() {
        static const std::string block = [] {
            std::string b;
            hpack::encode_literal(b, ":status", "200");
            hpack::encode_literal(b, "content-type", "application/grpc");
            return b;
        }();
        return block;
    }

    static const std::string& ok_trailers() {
        static const std::string block = [] {
            std::string b;
            hpack::encode_literal(b, "grpc-status", "0");
            return b;
        }();
        return block;
    }

    void send_response_headers(uint32_t sid, Stream& s) {
        if (s.headers_sent) return;
        send_header_block(sid, response_headers(), false);
        s.headers_sent = true;
    }

    void send_header_block(uint32_t sid, const std::string& block,
                           bool end_stream) {
        size_t off = 0;
        bool first = true;
        do {
            size_t n = std::min<size_t>(peer_max_frame_, block.size() - off);
            bool last = off + n == block.size();
            uint8_t flags = last ? END_HEADERS : 0;
            if (first && end_stream) flags |= END_STREAM;
            put_frame_header(out_, (uint32_t)n, first ? HEADERS : CONTINUATION,
                             flags, sid);
            out_.append(block, off, n);
            off += n;
            first = false;
        } while (off < block.size());
    }

    // Send as much of the stream's queued output as the windows allow;
    // trailers follow the last byte.
    void flush_stream(uint32_t sid) {
        Stream* s = find(sid);
        if (!s) return;
        for (;;) {
            while (s->pending_off < s->pending.size()) {
                int64_t avail = std::min<int64_t>(
                    std::min(s->send_window, conn_send_window_), peer_max_frame_);
                if (avail <= 0) return;   // WINDOW_UPDATE resumes us
                size_t n = std::min<size_t>((size_t)avail,
                                            s->pending.size() - s->pending_off);
                put_frame_header(out_, (uint32_t)n, DATA, 0, sid);
                out_.append(s->pending, s->pending_off, n);
                s->pending_off += n;
                s->send_window -= (int64_t)n;
                conn_send_window_ -= (int64_t)n;
            }
            s->pending.clear();
            s->pending_off = 0;
            if (!s->has_next) break;
            s->pending.swap(s->next_msg);
            s->next_msg.clear();
            s->has_next = false;
        }
        if (s->has_trailers) {
            send_header_block(sid, s->trailers, true);
            close_local(sid);
        }
    }

    void flush_all() {
        std::vector<uint32_t> ids;
        for (auto& kv : streams_)
            if (kv.second.pending_off < kv.second.pending.size() ||
                kv.second.has_trailers)
                ids.push_back(kv.first);
        std::sort(ids.begin(), ids.end());
        for (uint32_t sid : ids) {
            if (conn_send_window_ <= 0) break;
            flush_stream(sid);
        }
    }

    // We have sent END_STREAM. If the peer has not half-closed yet, tell it
    // to stop (RFC 7540 §8.1: RST_STREAM(NO_ERROR) after a full response).
    void close_local(uint32_t sid) {
        Stream* s = find(sid);
        if (!s) return;
        if (!s->remote_closed) send_rst(sid, NO_ERROR);
        erase_stream(sid);
    }

    void send_rst(uint32_t sid, uint32_t code) {
        put_frame_header(out_, 4, RST_STREAM, 0, sid);
        put_u32(out_, code);
    }

    void stream_error(uint32_t sid, uint32_t code) {
        send_rst(sid, code);
        erase_stream(sid);
    }

    void send_goaway(uint32_t code) {
        put_frame_header(out_, 8, GOAWAY, 0, 0);
        put_u32(out_, last_sid_);
        put_u32(out_, code);
        goaway_code_ = code;
    }

    void conn_error(uint32_t code) {
        if (dead_) return;
        send_goaway(code);
        streams_.clear();
        watch_streams_ = 0;
        dead_ = true;
    }

    void send_window_update(uint32_t sid, uint32_t inc) {
        put_frame_header(out_, 4, WINDOW_UPDATE, 0, sid);
        put_u32(out_, inc);
    }

    void end_watch_streams(int status) {
        std::vector<uint32_t> ids;
        for (auto& kv : streams_)
            if (kv.second.watch) ids.push_back(kv.first);
        for (uint32_t sid : ids) finish_stream(sid, status);
    }

    // ---- frames --------------------------------------------------------
    void on_frame(const FrameHeader& h, const uint8_t* p) {
        if (expect_cont_ && (h.type != CONTINUATION || h.stream != expect_cont_))
            return conn_error(PROTOCOL_ERROR);
        if (!got_settings_ && (h.type != SETTINGS || (h.flags & ACK)))
            return conn_error(PROTOCOL_ERROR);
        switch (h.type) {
        case DATA: return on_data(h, p);
        case HEADERS: return on_headers(h, p);
        case PRIORITY:
            if (h.stream == 0) return conn_error(PROTOCOL_ERROR);
            if (h.length != 5) {
                if (find(h.stream)) stream_error(h.stream, FRAME_SIZE_ERROR);
                else return conn_error(FRAME_SIZE_ERROR);
            }
            return;
        case RST_STREAM:
            if (h.stream == 0) return conn_error(PROTOCOL_ERROR);
            if (h.length != 4) return conn_error(FRAME_SIZE_ERROR);
            if (h.stream > last_sid_) return conn_error(PROTOCOL_ERROR);
            erase_stream(h.stream);
            return;
        case SETTINGS: return on_settings(h, p);
        case PUSH_PROMISE: return conn_error(PROTOCOL_ERROR);
        case PING:
            if (h.stream != 0) return conn_error(PROTOCOL_ERROR);
            if (h.length != 8) return conn_error(FRAME_SIZE_ERROR);
            if (!(h.flags & ACK)) {
                put_frame_header(out_, 8, PING, ACK, 0);
                out_.append((const char*)p, 8);
            }
            return;
        case GOAWAY:
            if (h.stream != 0) return conn_error(PROTOCOL_ERROR);
            if (h.length < 8) return conn_error(FRAME_SIZE_ERROR);
            peer_goaway_ = true;
            end_watch_streams(GRPC_UNAVAILABLE);
            return;
        case WINDOW_UPDATE: return on_window_update(h, p);
        case CONTINUATION:
            if (!expect_cont_) return conn_error(PROTOCOL_ERROR);
            if (hdr_buf_.size() + h.length > kMaxHeaderBlock)
                return conn_error(ENHANCE_YOUR_CALM);
            hdr_buf_.append((const char*)p, h.length);
            if (h.flags & END_HEADERS) {
                expect_cont_ = 0;
                headers_complete();
            }
            return;
        default:
            return;   // unknown frame types are ignored (RFC 7540 §4.1)
        }
    }

    void on_settings(const FrameHeader& h, const uint8_t* p) {
        if (h.stream != 0) return conn_error(PROTOCOL_ERROR);
        if (h.flags & ACK) {
            if (h.length != 0) return conn_error(FRAME_SIZE_ERROR);
            return;
        }
        if (h.length % 6) return conn_error(FRAME_SIZE_ERROR);
        for (uint32_t i = 0; i < h.length; i += 6) {
            uint32_t id = ((uint32_t)p[i] << 8) | p[i + 1];
            uint32_t v = get_u32(p + i + 2);
            switch (id) {
            case 2:   // ENABLE_PUSH
                if (v > 1) return conn_error(PROTOCOL_ERROR);
                break;
            case 4: { // INITIAL_WINDOW_SIZE: the delta applies to open streams
                if (v > (uint32_t)kMaxWindow) return conn_error(FLOW_CONTROL_ERROR);
                int64_t delta = (int64_t)v - peer_initial_window_;
                peer_initial_window_ = v;
                for (auto& kv : streams_) {
                    kv.second.send_window += delta;
                    if (kv.second.send_window > kMaxWindow)
                        return conn_error(FLOW_CONTROL_ERROR);
                }
                break;
            }
            case 5:   // MAX_FRAME_SIZE
                if (v < 16384 || v > 16777215) return conn_error(PROTOCOL_ERROR);
                peer_max_frame_ = v;
                break;
            default:  // HEADER_TABLE_SIZE (we never index), others: ignore
                break;
            }
        }
        got_settings_ = true;
        put_frame_header(out_, 0, SETTINGS, ACK, 0);
        flush_all();
    }

    void on_window_update(const FrameHeader& h, const uint8_t* p) {
        if (h.length != 4) return conn_error(FRAME_SIZE_ERROR);
        uint32_t inc = get_u32(p) & 0x7fffffffu;
        if (h.stream == 0) {
            if (inc == 0) return conn_error(PROTOCOL_ERROR);
            conn_send_window_ += inc;
            if (conn_send_window_ > kMaxWindow)
                return conn_error(FLOW_CONTROL_ERROR);
            flush_all();
            return;
        }
        if (h.stream > last_sid_) return conn_error(PROTOCOL_ERROR);
        Stream* s = find(h.stream);
        if (!s) return;   // closed: late frames are fine
        if (inc == 0) return stream_error(h.stream, PROTOCOL_ERROR);
        s->send_window += inc;
        if (s->send_window > kMaxWindow)
            return stream_error(h.stream, FLOW_CONTROL_ERROR);
        flush_stream(h.stream);
    }

    void on_data(const FrameHeader& h, const uint8_t* p) {
        if (h.stream == 0) return conn_error(PROTOCOL_ERROR);
        // Flow control counts the whole payload, padding included, and
        // counts it even for streams we have already closed.
        conn_recv_window_ -= h.length;
        if (conn_recv_window_ < 0) return conn_error(FLOW_CONTROL_ERROR);
        conn_recv_unacked_ += h.length;
        if (conn_recv_unacked_ >= kWindowSlack) {
            send_window_update(0, conn_recv_unacked_);
            conn_recv_window_ += conn_recv_unacked_;
            conn_recv_unacked_ = 0;
        }
        size_t n = h.length;
        if (!strip_padding(DATA, h.flags, p, n)) return conn_error(PROTOCOL_ERROR);
        Stream* s = find(h.stream);
        if (!s) {
            if (h.stream > last_sid_ || !(h.stream & 1))
                return conn_error(PROTOCOL_ERROR);   // idle stream
            return;                                   // closed: drop
        }
        if (s->remote_closed) return stream_error(h.stream, STREAM_CLOSED);
        s->recv_window -= h.length;
        if (s->recv_window < 0) return conn_error(FLOW_CONTROL_ERROR);
        const bool end = h.flags & END_STREAM;
        if (!end) {
            s->recv_unacked += h.length;
            if (s->recv_unacked >= kWindowSlack) {
                send_window_update(h.stream, s->recv_unacked);
                s->recv_window += s->recv_unacked;
                s->recv_unacked = 0;
            }
        }
        if (n) {
            s->body.append((const char*)p, n);
            if (s->body.size() >= 5) {
                const uint8_t* b = (const uint8_t*)s->body.data();
                uint32_t mlen = get_u32(b + 1);
                if (b[0] == 1)
                    return reject(h.stream, GRPC_UNIMPLEMENTED,
                                  "compressed request messages are not supported");
                if (b[0] != 0)
                    return reject(h.stream, GRPC_INTERNAL, "bad message prefix");
                if (mlen > kMaxMessage)
                    return reject(h.stream, GRPC_RESOURCE_EXHAUSTED,
                                  "request message too large");
                if (s->body.size() > 5 + (size_t)mlen)
                    return reject(h.stream, GRPC_INTERNAL,
                                  "more than one request message");
            }
        }
        if (end) {
            s->remote_closed = true;
            dispatch(h.stream);
        }
    }

    // Answer a request before the client has finished sending it.
    void reject(uint32_t sid, int status, const std::string& message) {
        reply_error(sid, status, message);   // closes + RST_STREAM(NO_ERROR)
    }

    void on_headers(const FrameHeader& h, const uint8_t* p) {
        if (h.stream == 0) return conn_error(PROTOCOL_ERROR);
        size_t n = h.length;
        if (!strip_padding(HEADERS, h.flags, p, n))
            return conn_error(PROTOCOL_ERROR);
        hdr_sid_ = h.stream;
        hdr_end_stream_ = h.flags & END_STREAM;
        hdr_buf_.assign((const char*)p, n);
        if (h.flags & END_HEADERS) headers_complete();
        else expect_cont_ = h.stream;
    }

    void headers_complete() {
        // Always decode: the dynamic table is connection state even when
        // the block belongs to a stream we no longer care about.
        std::vector<hpack::Header> hs;
        bool ok = decoder_.decode((const uint8_t*)hdr_buf_.data(),
                                  hdr_buf_.size(), hs);
        hdr_buf_.clear();
        if (!ok) return conn_error(COMPRESSION_ERROR);
        const uint32_t sid = hdr_sid_;
        if (!(sid & 1)) return conn_error(PROTOCOL_ERROR);
        if (Stream* s = find(sid)) {     // request trailers
            if (!hdr_end_stream_) return stream_error(sid, PROTOCOL_ERROR);
            if (s->remote_closed) return stream_error(sid, STREAM_CLOSED);
            s->remote_closed = true;
            return dispatch(sid);
        }
        if (sid <= last_sid_) return;    // closed stream: late trailers
        last_sid_ = sid;
        if (peer_goaway_ || shutting_down_ || streams_.size() >= kMaxStreams)
            return send_rst(sid, REFUSED_STREAM);

        std::string path, method, ctype;
        bool regular = false, malformed = false;
        for (auto& hd : hs) {
            if (hd.name.empty()) { malformed = true; break; }
            for (unsigned char c : hd.name)
                if (c >= 'A' && c <= 'Z') malformed = true;
            if (hd.name[0] == ':') {
                if (regular) malformed = true;
                if (hd.name == ":path") path = hd.value;
                else if (hd.name == ":method") method = hd.value;
                else if (hd.name != ":scheme" && hd.name != ":authority")
                    malformed = true;
            } else {
                regular = true;
                if (hd.name == "content-type") ctype = hd.value;
            }
        }
        if (malformed || path.empty() || method.empty())
            return send_rst(sid, PROTOCOL_ERROR);
        if (method != "POST" || ctype.compare(0, 16, "application/grpc") != 0) {
            std::string block;
            hpack::encode_literal(block, ":status",
                                  method != "POST" ? "405" : "415");
            send_header_block(sid, block, true);
            if (!hdr_end_stream_) send_rst(sid, NO_ERROR);
            return;
        }
        Stream& s = streams_[sid];
        s.path = std::move(path);
        s.send_window = peer_initial_window_;
        if (hdr_end_stream_) {
            s.remote_closed = true;
            dispatch(sid);
        }
    }

    void dispatch(uint32_t sid) {
        Stream* s = find(sid);
        if (!s) return;
        if (s->body.size() < 5)
            return reply_error(sid, GRPC_INTERNAL, "missing request message");
        uint32_t mlen = get_u32((const uint8_t*)s->body.data() + 1);
        if (s->body.size() != 5 + (size_t)mlen)
            return reply_error(sid, GRPC_INTERNAL, "truncated request message");
        std::string msg(s->body, 5);
        std::string path = s->path;
        std::string().swap(s->body);
        app_->on_rpc(*this, sid, path, msg);
    }

    App* app_;
    std::string in_, out_;
    bool preface_done_ = false;
    size_t preface_seen_ = 0;
    bool got_settings_ = false;
    bool dead_ = false;
    bool peer_goaway_ = false;
    bool shutting_down_ = false;
    uint32_t goaway_code_ = 0;
    uint32_t last_sid_ = 0;
    uint32_t expect_cont_ = 0;
    uint32_t hdr_sid_ = 0;
    bool hdr_end_stream_ = false;
    std::string hdr_buf_;
    hpack::Decoder decoder_;
    int64_t conn_send_window_ = kDefaultWindow;
    int64_t conn_recv_window_ = kDefaultWindow;
    uint32_t conn_recv_unacked_ = 0;
    int64_t peer_initial_window_ = kDefaultWindow;
    uint32_t peer_max_frame_ = 16384;
    std::unordered_map<uint32_t, Stream> streams_;
    size_t watch_streams_ = 0;
};

}  // namespace h2
}  // namespace kxdp
