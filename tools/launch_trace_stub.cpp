// Stand-in for the HIP runtime entry points that hipcc's host-side `<<<>>>` stubs call: it records launches and runs nothing, so the host
// dispatch of a .hip file can be traced on a machine without a GPU.  Linked (with clang++, without libamdhip64) into a stand-alone
// program such as tools/gn_launch_trace.cpp, next to the host objects under test; never a shared library, never preloaded.
//
// Argument sizes and offsets come from the code object's own kernel metadata: LAUNCH_TRACE_NOTES names the text that
// `llvm-readelf --notes` prints for the device code object (amdhsa.kernels: .args / .offset / .size / .value_kind / .name).
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

namespace {
struct Arg { size_t offset, size; };
// function-local statics: registration runs from a static constructor of the .hip object, possibly before this file's own
std::map<const void*, std::string>& names() { static std::map<const void*, std::string> m; return m; }
const std::vector<Arg>* args_of(const std::string& kernel) {
    static std::map<std::string, std::vector<Arg>> table = [] {
        std::map<std::string, std::vector<Arg>> t;
        const char* path = getenv("LAUNCH_TRACE_NOTES");
        std::ifstream in(path ? path : "");
        std::vector<Arg> cur;
        for (std::string l; std::getline(in, l);) {
            const size_t ind = l.find_first_not_of(" -"), colon = l.find(':');
            if (ind == std::string::npos || colon == std::string::npos) continue;
            const size_t v0 = l.find_first_not_of(' ', colon + 1);
            const std::string key = l.substr(ind, colon - ind), val = v0 == std::string::npos ? "" : l.substr(v0);
            if (key == ".offset") cur.push_back({std::stoul(val), 0});
            else if (key == ".size" && !cur.empty()) cur.back().size = std::stoul(val);
            else if (key == ".value_kind" && val.rfind("hidden_", 0) == 0) cur.pop_back();     // the explicit arguments only
            else if (key == ".name" && ind == 4) { t[val] = cur; cur.clear(); }                // kernel level (argument names sit deeper)
        }
        return t;
    }();
    const auto it = table.find(kernel);
    return it == table.end() ? nullptr : &it->second;
}
std::string g_log;
struct Pad { std::string kernel_part; size_t arg_size, offset, len; };
std::vector<Pad> g_pads;
bool is_padding(const char* kernel, size_t arg_size, size_t b) {
    for (const Pad& p : g_pads)
        if (p.arg_size == arg_size && b >= p.offset && b < p.offset + p.len && strstr(kernel, p.kernel_part.c_str())) return true;
    return false;
}
struct { dim3 grid, block; size_t lds; hipStream_t stream; } g_cfg;
void logf(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_log += buf;
}
const char* name_of(const void* f) {
    const auto it = names().find(f);
    return it == names().end() ? "?" : it->second.c_str();
}
}  // namespace

// what the stand-in saw since the last call (declared by the tracing program)
std::string launch_trace_take() { std::string s; s.swap(g_log); return s; }
// padding bytes of a struct passed by value (indeterminate on the host): printed as "--" in every by-value argument of that size
void launch_trace_padding(size_t arg_size, size_t offset, size_t len) { g_pads.push_back({"", arg_size, offset, len}); }
// the same for bytes a launch leaves unset, in the kernels whose name contains kernel_part only; launch_trace_unmask drops that part's ranges
void launch_trace_mask(const char* kernel_part, size_t arg_size, size_t offset, size_t len) { g_pads.push_back({kernel_part, arg_size, offset, len}); }
void launch_trace_unmask(const char* kernel_part) {
    for (size_t i = g_pads.size(); i-- > 0;)
        if (g_pads[i].kernel_part == kernel_part) g_pads.erase(g_pads.begin() + i);
}

extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, void*, void*, dim3*, dim3*, int*) { names()[host_fn] = device_name; }
void __hipRegisterVar(void**, void*, char*, const char*, int, size_t, int, int) {}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t stream) { g_cfg = {grid, block, lds, stream}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* stream) {
    *grid = g_cfg.grid; *block = g_cfg.block; *lds = g_cfg.lds; *stream = g_cfg.stream;
    return hipSuccess;
}
hipError_t hipLaunchKernel(const void* f, dim3 grid, dim3 block, void** args, size_t lds, hipStream_t stream) {
    const char* name = name_of(f);
    logf(" launch=%s grid=%u,%u,%u block=%u,%u,%u lds=%zu stream=%p args=", name, grid.x, grid.y, grid.z, block.x, block.y, block.z, lds, (void*)stream);
    const std::vector<Arg>* layout = args_of(name);
    if (!layout) { g_log += "no-metadata"; return hipSuccess; }
    for (size_t i = 0; i < layout->size(); ++i) {
        logf("%s%zu:", i ? "," : "", (*layout)[i].offset);
        for (size_t b = 0; b < (*layout)[i].size; ++b) {
            if (is_padding(name, (*layout)[i].size, b)) { g_log += "--"; continue; }
            const unsigned char v = ((const unsigned char*)args[i])[b];
            g_log += "0123456789abcdef"[v >> 4];
            g_log += "0123456789abcdef"[v & 15];
        }
    }
    return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void* f, hipFuncAttribute attr, int value) {
    logf(" attr=%s:%d:%d", name_of(f), (int)attr, value);
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "stub"; }
}
