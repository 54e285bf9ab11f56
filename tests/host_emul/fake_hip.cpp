// fake_hip.cpp -- a HIP runtime for the host half of the library alone (tests/test_host_abi_cpu.py, not a product path).
// Device memory is malloc (so AddressSanitizer bounds the host side of every copy and LeakSanitizer sees a forgotten free),
// nothing runs on a device, and every call that allocates, frees, copies, waits, records or launches is written to an event
// list that abi_host.cpp prints under the ABI call that caused it.
#include <hip/hip_runtime_api.h>

#include <cxxabi.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

std::vector<std::string> &fake_hip_events() {
    static std::vector<std::string> ev;
    return ev;
}

namespace {

// (function-local statics: the registration calls of the library's files run before this file's static constructors)
std::map<const void *, std::string> &kernel_names() {
    static std::map<const void *, std::string> names;
    return names;
}
std::map<void *, size_t> &blocks() {
    static std::map<void *, size_t> b;
    return b;
}

struct Config {
    dim3 grid, block;
    size_t lds;
    hipStream_t st;
};
std::vector<Config> stack;
bool pending = false;       // a pushed launch configuration that no hipLaunchKernel has named yet
Config pending_cfg;
std::string attr_name;      // kernel of the last hipFuncSetAttribute since the last launch

std::string launch_line(const std::string &name, const Config &c) {
    char buf[160];
    snprintf(buf, sizeof(buf), " grid %u,%u,%u block %u,%u,%u lds %zu", c.grid.x, c.grid.y, c.grid.z, c.block.x, c.block.y, c.block.z, c.lds);
    return "launch " + name + buf;
}

// A kernel launched through a function-pointer variable never reaches hipLaunchKernel in this link: its configuration is
// logged when the next event (or the end of the call) arrives, named by the hipFuncSetAttribute just before it, if any
void flush() {
    if (!pending) return;
    pending = false;
    fake_hip_events().push_back(launch_line(attr_name.empty() ? "?" : attr_name, pending_cfg));
    attr_name.clear();
}

void event(const char *what, size_t bytes) {
    flush();
    fake_hip_events().push_back(std::string(what) + " " + std::to_string(bytes));
}
void event(const char *what) {
    flush();
    fake_hip_events().push_back(what);
}

std::string name_of(const void *f) {
    auto it = kernel_names().find(f);
    return it == kernel_names().end() ? "?" : it->second;
}

}  // namespace

void fake_hip_flush() { flush(); }

extern "C" {

void **__hipRegisterFatBinary(const void *) {
    static void *handle;
    return &handle;
}
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host, char *, const char *device_name, unsigned, void *, void *, void *, void *, int *) {
    int status = 0;
    char *d = abi::__cxa_demangle(device_name, nullptr, nullptr, &status);
    std::string n = status == 0 && d ? d : device_name;
    free(d);
    // "void mulut::k<1, 2>(mulut::Args)" -> "k<1, 2>"
    size_t depth = 0, cut = n.size();
    for (size_t i = 0; i < n.size(); ++i) {
        if (n[i] == '<') ++depth;
        else if (n[i] == '>') --depth;
        else if (n[i] == '(' && depth == 0) {
            cut = i;
            break;
        }
    }
    n = n.substr(0, cut);
    if (n.compare(0, 5, "void ") == 0) n = n.substr(5);
    for (size_t p; (p = n.find("mulut::")) != std::string::npos;) n.erase(p, 7);
    kernel_names()[host] = n;
}
void __hipRegisterVar(void **, void *, char *, char *, int, size_t, int, int) {}
void __hipRegisterManagedVar(void *, void **, void *, const char *, size_t, unsigned) {}

hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t st) {
    flush();
    pending_cfg = Config{grid, block, lds, st};
    pending = true;
    stack.push_back(pending_cfg);
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *lds, hipStream_t *st) {
    if (stack.empty()) return hipErrorInvalidValue;
    const Config c = stack.back();
    stack.pop_back();
    *grid = c.grid; *block = c.block; *lds = c.lds; *st = c.st;
    return hipSuccess;
}
hipError_t hipLaunchKernel(const void *f, dim3 grid, dim3 block, void **, size_t lds, hipStream_t st) {
    pending = false;
    attr_name.clear();
    fake_hip_events().push_back(launch_line(name_of(f), Config{grid, block, lds, st}));
    return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void *f, hipFuncAttribute, int value) {
    flush();
    attr_name = name_of(f);
    fake_hip_events().push_back("lds_limit " + attr_name + " " + std::to_string(value));
    return hipSuccess;
}

hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : hipErrorInvalidDevice; }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t *p, int) {
    memset(p, 0, sizeof(*p));
    p->multiProcessorCount = 256;
    return hipSuccess;
}
hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t, int) { *v = 256; return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "fake"; }
hipError_t hipGetLastError(void) { return hipSuccess; }

hipError_t hipMalloc(void **p, size_t n) {
    *p = malloc(n ? n : 1);
    blocks()[*p] = n;
    event("malloc", n);
    return hipSuccess;
}
hipError_t hipFree(void *p) {
    if (!p) return hipSuccess;
    auto it = blocks().find(p);
    if (it == blocks().end()) {
        event("free of an unknown pointer");
        return hipErrorInvalidValue;
    }
    event("free", it->second);
    blocks().erase(it);
    free(p);
    return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind) {
    memcpy(dst, src, n);
    event("memcpy", n);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind, hipStream_t) {
    memcpy(dst, src, n);
    event("memcpy", n);
    return hipSuccess;
}
hipError_t hipMemset(void *p, int v, size_t n) {
    memset(p, v, n);
    event("memset", n);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) {
    memset(p, v, n);
    event("memset", n);
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { event("wait device"); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { event("wait stream"); return hipSuccess; }

hipError_t hipEventCreate(hipEvent_t *e) {
    *e = (hipEvent_t)malloc(1);
    event("event_create");
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    free(e);
    event("event_destroy");
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { event("event_record"); return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { event("wait event"); return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.0f; return hipSuccess; }

}  // extern "C"
