// The library's one device allocator: acc_malloc / acc_free (internal.h).  With the debug switch off they are hipMalloc /
// hipFree.  With accbpg_debug_guard_bands(bytes) on, every allocation is surrounded by `bytes` of a NaN sentinel and
// entered in the registry of guard_alloc.hpp; accbpg_debug_guard_check compares the bands of the live ones.  This is
// the only file of the library that names hipMalloc / hipFree (tests/test_guard_cpu.py checks the others).
#include "guard_alloc.hpp"
#include "internal.h"

namespace accbpg {
namespace {

int raw_alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
int raw_release(void* p) { return (int)hipFree(p); }
int raw_upload(void* dst, const void* src, size_t bytes) { return (int)hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
int raw_download(void* dst, const void* src, size_t bytes) {
    return (int)hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
}

guard::Registry& registry() {
    static guard::Registry* r = new guard::Registry(guard::RawOps{raw_alloc, raw_release, raw_upload, raw_download});
    return *r;    // never destroyed: a handle may still be freed while the process's static destructors run
}

}  // namespace

hipError_t acc_malloc(void** p, size_t bytes, const char* label) {
    guard::Registry& r = registry();
    if (r.band() == 0) return hipMalloc(p, bytes);
    return (hipError_t)r.allocate(p, bytes, label);
}

hipError_t acc_free(void* p) {
    guard::Registry& r = registry();
    if (r.live() == 0) return hipFree(p);
    return (hipError_t)r.release(p);
}

}  // namespace accbpg

extern "C" int accbpg_debug_guard_bands(int64_t bytes) {
    if (accbpg::registry().set_band(bytes) != 0) {
        accbpg::set_last_error("accbpg_debug_guard_bands: %lld is not a non-negative multiple of 4096", (long long)bytes);
        return ACCBPG_ERR_ARG;
    }
    return ACCBPG_OK;
}

extern "C" int accbpg_debug_guard_check(int64_t* out3) {
    if (!out3) {
        accbpg::set_last_error("accbpg_debug_guard_check: out3 is null");
        return ACCBPG_ERR_ARG;
    }
    ACC_HIP(hipDeviceSynchronize());
    accbpg::guard::Damage first;
    const int rc = accbpg::registry().check(out3, &first);
    if (rc != 0) {
        accbpg::set_last_error("accbpg_debug_guard_check: copying a band -> %s", hipGetErrorString((hipError_t)rc));
        return ACCBPG_ERR_HIP;
    }
    if (first.any) accbpg::set_last_error("%s", accbpg::guard::Registry::describe(first).c_str());
    return ACCBPG_OK;
}
