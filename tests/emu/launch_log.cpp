// TEST INFRASTRUCTURE: the launch log of the emulation.  hipLaunchKernelGGL (include/hip/hip_runtime.h) records the spelling of
// every kernel expression it launches, in order, so that a test can assert which kernel a call of the C ABI reached; beside it
// the instantiation with its template arguments resolved and the block size ("radon_fwd_tiled_kernel<8, false, 9> x512").
#include <cstdlib>
#include <cstring>
#include <cxxabi.h>
#include <string>
#include <vector>

namespace {
std::vector<std::string> g_launches, g_instances;

// the mangled name of emu::KernelTag<&kernel> -> "kernel<8, false, 9>"; a spelling (no instantiation logged) passes unchanged
std::string instance_of(const char* sig) {
    int st = 1;
    char* dm = abi::__cxa_demangle(sig, nullptr, nullptr, &st);
    if (st != 0 || !dm) return sig;
    std::string s(dm);
    std::free(dm);
    for (const char* drop : {"(anonymous namespace)::", "dinv::"})
        for (size_t p; (p = s.find(drop)) != std::string::npos;) s.erase(p, std::strlen(drop));
    // "emu::KernelTag<&(void name<args>(params))>" for a template, "emu::KernelTag<&name>" for a plain function
    size_t b = s.find("&(");
    if (b == std::string::npos) {
        b = s.find('&');
        return b == std::string::npos || s.back() != '>' ? s : s.substr(b + 1, s.size() - b - 2);
    }
    b = s.find(' ', b) + 1;                 // past the return type
    int depth = 0;
    size_t e = b;
    for (; e < s.size(); ++e) {
        if (s[e] == '<') ++depth;
        else if (s[e] == '>') --depth;
        else if (s[e] == '(' && depth == 0) break;
    }
    return s.substr(b, e - b);
}
}  // namespace

extern "C" void dinv_emu_log_launch(const char* kernel) { g_launches.emplace_back(kernel); }
extern "C" void dinv_emu_log_instance(const char* signature, unsigned block) {
    g_instances.emplace_back(instance_of(signature) + " x" + std::to_string(block));
}
extern "C" void dinv_emu_launch_log_reset() { g_launches.clear(); g_instances.clear(); }
extern "C" int dinv_emu_launch_log_count() { return (int)g_launches.size(); }
extern "C" const char* dinv_emu_launch_log_name(int i) {
    return i >= 0 && i < (int)g_launches.size() ? g_launches[i].c_str() : nullptr;
}
extern "C" const char* dinv_emu_launch_log_instance(int i) {
    return i >= 0 && i < (int)g_instances.size() ? g_instances[i].c_str() : nullptr;
}
