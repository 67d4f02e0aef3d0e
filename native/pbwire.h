// Minimal protobuf wire helpers: varints and length-delimited fields, just
// enough for the DevicePlugin v1beta1 messages the native server touches
// (AllocateRequest in, AllocateResponse out). No pybind11 / Python.h.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace kxdp {
namespace pb {

inline void put_varint(std::string& out, uint64_t v) {
    while (v >= 128) {
        out.push_back((char)((v & 0x7f) | 0x80));
        v >>= 7;
    }
    out.push_back((char)v);
}

// tag + length + bytes for a length-delimited field (wire type 2)
inline void put_bytes(std::string& out, uint32_t field, const char* p, size_t n) {
    put_varint(out, ((uint64_t)field << 3) | 2);
    put_varint(out, n);
    out.append(p, n);
}

inline void put_bytes(std::string& out, uint32_t field, const std::string& s) {
    put_bytes(out, field, s.data(), s.size());
}

// map<string,string> entry as field `field`: {1: key, 2: value}
inline void put_map_entry(std::string& out, uint32_t field,
                          const std::string& key, const std::string& value) {
    std::string e;
    put_bytes(e, 1, key);
    put_bytes(e, 2, value);
    put_bytes(out, field, e);
}

struct Reader {
    const uint8_t* p;
    const uint8_t* end;

    Reader(const void* data, size_t n)
        : p((const uint8_t*)data), end((const uint8_t*)data + n) {}

    bool done() const { return p >= end; }

    bool varint(uint64_t& v) {
        v = 0;
        for (int shift = 0; shift < 64; shift += 7) {
            if (p >= end) return false;
            uint8_t b = *p++;
            v |= (uint64_t)(b & 0x7f) << shift;
            if (!(b & 0x80)) return true;
        }
        return false;
    }

    // Next field header; false on malformed input.
    bool tag(uint32_t& field, uint32_t& wire) {
        uint64_t t;
        if (!varint(t) || (t >> 3) == 0 || (t >> 3) > 0x1fffffff) return false;
        field = (uint32_t)(t >> 3);
        wire = (uint32_t)(t & 7);
        return true;
    }

    bool bytes(const uint8_t*& data, size_t& n) {
        uint64_t len;
        if (!varint(len) || len > (uint64_t)(end - p)) return false;
        data = p;
        n = (size_t)len;
        p += len;
        return true;
    }

    // Skip a field of the given wire type (groups are rejected).
    bool skip(uint32_t wire) {
        uint64_t v;
        const uint8_t* d;
        size_t n;
        switch (wire) {
        case 0: return varint(v);
        case 1: if (end - p < 8) return false; p += 8; return true;
        case 2: return bytes(d, n);
        case 5: if (end - p < 4) return false; p += 4; return true;
        default: return false;
        }
    }
};

// AllocateRequest{ repeated ContainerAllocateRequest container_requests = 1 }
// ContainerAllocateRequest{ repeated string devices_ids = 1 }
inline bool parse_allocate_request(
    const std::string& msg, std::vector<std::vector<std::string>>& out) {
    Reader r(msg.data(), msg.size());
    while (!r.done()) {
        uint32_t field, wire;
        if (!r.tag(field, wire)) return false;
        if (field == 1 && wire == 2) {
            const uint8_t* d;
            size_t n;
            if (!r.bytes(d, n)) return false;
            out.emplace_back();
            Reader c(d, n);
            while (!c.done()) {
                uint32_t cf, cw;
                if (!c.tag(cf, cw)) return false;
                if (cf == 1 && cw == 2) {
                    const uint8_t* s;
                    size_t sn;
                    if (!c.bytes(s, sn)) return false;
                    out.back().emplace_back((const char*)s, sn);
                } else if (!c.skip(cw)) {
                    return false;
                }
            }
        } else if (!r.skip(wire)) {
            return false;
        }
    }
    return true;
}

}  // namespace pb
}  // namespace kxdp
