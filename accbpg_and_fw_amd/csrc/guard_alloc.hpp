// Guard bands around the library's own device allocations (a debug switch): the band arithmetic and the registry of
// banded allocations, free of HIP.  The raw operations -- allocate, free, copy to and from the memory the allocations
// live in -- are passed in (guard_alloc.hip passes hipMalloc / hipFree / hipMemcpy; tests/test_guard_cpu.py passes
// malloc / free / memcpy and runs the header under the host sanitizers).
//
// A banded allocation of `bytes` with band width B (a multiple of 4096):
//
//     base                 user = base + B            user + bytes          base + total
//     |<----- front band ----->|<------ user region ------>|<------ back band ------>|
//
// total = B + round_up(bytes, 4096) + B, so the back band holds B bytes and the remainder of the user region's last
// page.  Both bands hold the eight bytes of SENTINEL over and over, in phase with base (byte i of the allocation is byte
// i % 8 of the sentinel; B % 8 == 0, so the phase is the same seen from user).  The user region is left as the raw
// allocator gave it.  user keeps the alignment of base up to 4096 bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace accbpg {
namespace guard {

constexpr uint64_t SENTINEL = 0x7FF8A5A5A5A5A5A5ull;    // a quiet NaN with a payload
constexpr size_t PAGE = 4096;

// every operation returns 0 on success, else a code of the caller's that the registry hands back unchanged
struct RawOps {
    int (*alloc)(void** p, size_t bytes);
    int (*release)(void* p);
    int (*upload)(void* dst, const void* host_src, size_t bytes);      // synchronous
    int (*download)(void* host_dst, const void* src, size_t bytes);    // synchronous, behind all work in flight
};

struct Layout {
    size_t front = 0;   // bytes of band in front of the user region
    size_t back = 0;    // bytes of band behind it (>= front)
    size_t total = 0;   // front + bytes + back
};

inline size_t round_up(size_t v, size_t to) { return (v + to - 1) / to * to; }
inline bool band_ok(int64_t band) { return band >= 0 && band % (int64_t)PAGE == 0; }
inline Layout layout(size_t bytes, size_t band) {
    Layout l;
    l.front = band;
    l.back = band + (round_up(bytes, PAGE) - bytes);
    l.total = l.front + bytes + l.back;
    return l;
}
// byte of the sentinel pattern at `offset` from the base of an allocation
inline unsigned char pattern_byte(size_t offset) { return (unsigned char)(SENTINEL >> (8 * (offset % 8))); }

enum Side { FRONT = 0, BACK = 1 };
struct Damage {         // the first damaged band of a check
    bool any = false;
    std::string label;
    Side side = FRONT;
    long long offset = 0;   // FRONT: -k, the byte k bytes in front of the user pointer; BACK: +k, the byte k bytes past
                            // the end of the user region (0 = the first byte behind it)
};
// first byte of a band's host copy that left the pattern (or -1), and how many did; `phase` = offset of the band's first
// byte from the base of its allocation
inline long long compare_band(const unsigned char* copy, size_t bytes, size_t phase, long long* damaged) {
    long long first = -1;
    for (size_t i = 0; i < bytes; ++i) {
        if (copy[i] != pattern_byte(phase + i)) {
            if (first < 0) first = (long long)i;
            ++*damaged;
        }
    }
    return first;
}

class Registry {
public:
    explicit Registry(const RawOps& ops) : ops_(ops) {}

    // width of the bands of the allocations made from now on (0: none); -1 for a width that is no multiple of 4096
    int set_band(int64_t bytes) {
        if (!band_ok(bytes)) return -1;
        band_.store((size_t)bytes);
        return 0;
    }
    size_t band() const { return band_.load(); }
    size_t live() const { return live_.load(); }

    int allocate(void** p, size_t bytes, const char* label) {
        const size_t band = band_.load();
        if (band == 0 || bytes == 0) return ops_.alloc(p, bytes);      // nothing added with the switch off
        const Layout l = layout(bytes, band);
        void* base = nullptr;
        int rc = ops_.alloc(&base, l.total);
        if (rc != 0) return rc;
        unsigned char* b = static_cast<unsigned char*>(base);
        std::vector<unsigned char> pat(l.back);
        for (size_t i = 0; i < l.front; ++i) pat[i] = pattern_byte(i);
        rc = ops_.upload(b, pat.data(), l.front);
        if (rc == 0) {
            const size_t phase = l.front + bytes;
            for (size_t i = 0; i < l.back; ++i) pat[i] = pattern_byte(phase + i);
            rc = ops_.upload(b + phase, pat.data(), l.back);
        }
        if (rc != 0) {
            ops_.release(base);
            return rc;
        }
        Entry e;
        e.base = base;
        e.bytes = bytes;
        e.lay = l;
        e.label = label ? label : "?";
        void* user = b + l.front;
        {
            std::lock_guard<std::mutex> g(mu_);
            live_map_[user] = e;
            live_.store(live_map_.size());
        }
        *p = user;
        return 0;
    }

    int release(void* p) {
        if (p && live_.load() != 0) {
            void* base = nullptr;
            {
                std::lock_guard<std::mutex> g(mu_);
                auto it = live_map_.find(p);
                if (it != live_map_.end()) {
                    base = it->second.base;
                    live_map_.erase(it);
                    live_.store(live_map_.size());
                }
            }
            if (base) return ops_.release(base);
        }
        return ops_.release(p);     // allocated with the switch off (or null)
    }

    // out3 = {live banded allocations, damaged bands, damaged bytes}; first = the first damaged band in address order
    int check(int64_t out3[3], Damage* first) {
        std::lock_guard<std::mutex> g(mu_);
        out3[0] = (int64_t)live_map_.size();
        out3[1] = out3[2] = 0;
        if (first) *first = Damage();
        std::vector<unsigned char> copy;
        for (const auto& kv : live_map_) {
            const Entry& e = kv.second;
            const unsigned char* b = static_cast<const unsigned char*>(e.base);
            for (int side = 0; side < 2; ++side) {
                const size_t phase = side == FRONT ? 0 : e.lay.front + e.bytes;
                const size_t len = side == FRONT ? e.lay.front : e.lay.back;
                copy.resize(len);
                const int rc = ops_.download(copy.data(), b + phase, len);
                if (rc != 0) return rc;
                long long bad = 0;
                const long long at = compare_band(copy.data(), len, phase, &bad);
                if (at < 0) continue;
                out3[1] += 1;
                out3[2] += bad;
                if (first && !first->any) {
                    first->any = true;
                    first->label = e.label;
                    first->side = (Side)side;
                    first->offset = side == FRONT ? at - (long long)e.lay.front : at;
                }
            }
        }
        return 0;
    }

    static std::string describe(const Damage& d) {
        if (!d.any) return "";
        char buf[256];
        snprintf(buf, sizeof buf, "guard band damaged: %s, %s, byte %+lld from the user region's %s", d.label.c_str(),
                 d.side == FRONT ? "front" : "back", d.offset, d.side == FRONT ? "start" : "end");
        return buf;
    }

private:
    struct Entry {
        void* base = nullptr;
        size_t bytes = 0;
        Layout lay;
        std::string label;
    };
    RawOps ops_;
    std::atomic<size_t> band_{0};
    std::atomic<size_t> live_{0};
    std::mutex mu_;
    std::map<void*, Entry> live_map_;
};

}  // namespace guard
}  // namespace accbpg
