// launch_args.cpp -- which kernel every launch site of the fp32 quantize / min-max family picks, with what grid, workgroup and
// DYNAMIC shared memory (the sharedMemBytes launch argument a kernel trace does not show), without a GPU.
//
//   g++ -std=c++17 -rdynamic -I include tools/launch_args.cpp -ldl -o launch_args
//   ./launch_args fp8-quantization_amd/csrc/libfp8q_hip.so > new.txt ; ./launch_args /path/to/parent/libfp8q_hip.so > old.txt
//
// The program defines the handful of HIP runtime entry points the library imports (kernel registration, the <<< >>> call
// configuration, hipLaunchKernel) itself -- their signatures and Dim3 are copied from the runtime's ABI: check them when ROCm
// changes.  A program's own symbols come first in the lookup order, so the library loaded with dlopen registers its
// kernels here and "launches" them here: nothing runs, every launch is printed.  The entry points are
// called with made-up device addresses (the host code of these routes only looks at their alignment) at the shapes of
// tools/route_shapes.py plus the ones that matter for the LDS sizing; the calibration step (fp8q_quantize_select_f32, no
// dynamic LDS) is left to the trace.  Two builds give two files; diff them.
#include <cxxabi.h>
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <string>
#include <vector>

#include "fp8q.h"

struct Dim3 {
    unsigned x, y, z;
};

static std::map<const void *, std::string> g_names;
static Dim3 g_grid, g_block;
static size_t g_shmem;
static void *g_stream;

static std::string short_name(const char *mangled)
{
    int st = 0;
    char *d = abi::__cxa_demangle(mangled, nullptr, nullptr, &st);
    std::string s = st == 0 && d ? d : mangled;
    free(d);
    const std::string anon = "(anonymous namespace)::";
    for (size_t p; (p = s.find(anon)) != std::string::npos;) s.erase(p, anon.size());
    if (s.rfind("void ", 0) == 0) s.erase(0, 5);
    int depth = 0;   // cut the argument list: the first '(' outside template brackets
    for (size_t i = 0; i < s.size(); ++i) {
        if (s[i] == '<') ++depth;
        if (s[i] == '>') --depth;
        if (s[i] == '(' && depth == 0) return s.substr(0, i);
    }
    return s;
}

extern "C" {
void **__hipRegisterFatBinary(const void *)
{
    static void *dummy;
    return &dummy;
}
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host_fn, char *, const char *device_name, unsigned, void *, void *, void *, void *, int *)
{
    g_names[host_fn] = short_name(device_name);
}
void __hipRegisterVar(void **, void *, char *, char *, int, size_t, int, int) {}
int __hipPushCallConfiguration(Dim3 grid, Dim3 block, size_t shmem, void *stream)
{
    g_grid = grid, g_block = block, g_shmem = shmem, g_stream = stream;
    return 0;
}
int __hipPopCallConfiguration(Dim3 *grid, Dim3 *block, size_t *shmem, void **stream)
{
    *grid = g_grid, *block = g_block, *shmem = g_shmem, *stream = g_stream;
    return 0;
}
int hipLaunchKernel(const void *fn, Dim3 grid, Dim3 block, void **, size_t shmem, void *)
{
    const auto it = g_names.find(fn);
    printf("    %-50s grid %u x %u x %u  wg %u  dynamic LDS %zu\n", it == g_names.end() ? "?" : it->second.c_str(), grid.x, grid.y,
           grid.z, block.x, shmem);
    return 0;
}
int hipGetLastError(void) { return 0; }
const char *hipGetErrorString(int) { return "stub"; }
int hipFuncSetAttribute(const void *, int, int) { return 0; }
int hipMemcpy(void *, const void *, size_t, int) { return 0; }
int hipMemsetAsync(void *, int, size_t, void *) { return 0; }
int hipStreamSynchronize(void *) { return 0; }
}

static void *g_lib;
template <class F>
static F sym(const char *name)
{
    void *p = dlsym(g_lib, name);
    if (!p) {
        fprintf(stderr, "missing %s\n", name);
        exit(2);
    }
    return reinterpret_cast<F>(p);
}

// made-up device addresses: 16-byte aligned, `off` floats further
static float *X(int off = 0) { return reinterpret_cast<float *>(0x100000000ull) + off; }
static float *Y(int off = 0) { return reinterpret_cast<float *>(0x200000000ull) + off; }
static float *MV() { return reinterpret_cast<float *>(0x300000000ull); }
static float *R(int i) { return reinterpret_cast<float *>(0x400000000ull + 0x10000000ull * i); }
static uint8_t *CODES(int off = 0) { return reinterpret_cast<uint8_t *>(0x500000000ull) + off; }

int main(int argc, char **argv)
{
    if (argc != 2) return fprintf(stderr, "usage: %s libfp8q_hip.so\n", argv[0]), 2;
    g_lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!g_lib) return fprintf(stderr, "%s\n", dlerror()), 2;
    auto quantize = sym<decltype(&fp8q_quantize_f32)>("fp8q_quantize_f32");
    auto quantize_dm = sym<decltype(&fp8q_quantize_dm_f32)>("fp8q_quantize_dm_f32");
    auto quantize_ds = sym<decltype(&fp8q_quantize_ds_f32)>("fp8q_quantize_ds_f32");
    auto quantize_dms = sym<decltype(&fp8q_quantize_dms_f32)>("fp8q_quantize_dms_f32");
    auto minmax = sym<decltype(&fp8q_minmax_f32)>("fp8q_minmax_f32");
    auto ws_bytes = sym<decltype(&fp8q_minmax_workspace_bytes)>("fp8q_minmax_workspace_bytes");
    auto mmq = sym<decltype(&fp8q_minmax_quantize_f32)>("fp8q_minmax_quantize_f32");
    auto encode = sym<decltype(&fp8q_encode_u8)>("fp8q_encode_u8");
    auto decode = sym<decltype(&fp8q_decode_u8)>("fp8q_decode_u8");
    auto multi_q = sym<decltype(&fp8q_multi_quantize_f32)>("fp8q_multi_quantize_f32");
    auto multi_e = sym<decltype(&fp8q_multi_encode_u8)>("fp8q_multi_encode_u8");
    auto multi_d = sym<decltype(&fp8q_multi_decode_u8)>("fp8q_multi_decode_u8");
    auto multi_mmq = sym<decltype(&fp8q_multi_minmax_quantize_f32)>("fp8q_multi_minmax_quantize_f32");
    auto multi_mme = sym<decltype(&fp8q_multi_minmax_encode_u8)>("fp8q_multi_minmax_encode_u8");
    auto copy = sym<decltype(&fp8q_copy_f32)>("fp8q_copy_f32");
    int rc = 0;
#define CALL(what, expr)                  \
    do {                                  \
        printf("%s\n", what);             \
        const int r_ = (expr);            \
        if (r_) printf("    rc %d\n", r_), rc = 1; \
    } while (0)
    struct Shape {
        int64_t C, inner;
    };
    // (mbits, n_bits): E5M2 has 33-entry tables, E4M3 17, M = 6 three: the LDS per table row differs
    const float widths[] = {2.0f, 3.0f, 6.0f};
    char what[256];
    // per tensor: cached small / cached / nontemporal, aligned and not
    for (int64_t n : {(int64_t)4101, ((int64_t)8 << 20) + 4, ((int64_t)16 << 20) + 4, ((int64_t)64 << 20) + 4})
        for (int off : {0, 1}) {
            snprintf(what, sizeof what, "quantize per tensor n=%lld y+%d", (long long)n, off);
            CALL(what, quantize(X(), Y(off), 1, n, MV(), 1, 3.0f, 8, 1, nullptr));
        }
    CALL("copy n=20480", copy(X(), Y(), 20480, nullptr));
    CALL("copy n=2^26+4096", copy(X(), Y(), ((int64_t)1 << 26) + 4096, nullptr));
    // per channel K1: flat, direct (misaligned; no table), 2-D rows; big enough for the nontemporal variants too
    const Shape k1[] = {{4096, 147}, {64, 3}, {4096, 4}, {4096, 32}, {30000, 1152}, {100000, 576}, {2097152, 147}, {1000, 2047}, {8, 4608}, {70000, 4608}};
    for (const Shape &s : k1)
        for (float mb : widths)
            for (int off : {0, 1}) {
                snprintf(what, sizeof what, "quantize per channel [%lld,%lld] M=%g x,y+%d", (long long)s.C, (long long)s.inner, mb, off);
                CALL(what, quantize(X(off), Y(off), s.C, s.inner, MV(), s.C, mb, 8, 1, nullptr));
            }
    // format selected on the device
    const uint8_t *flag = CODES();
    for (const Shape &s : {Shape{1, 4101}, Shape{96, 9}, Shape{8, 4608}, Shape{1, ((int64_t)16 << 20) + 4}})
        for (int off : {0, 1}) {
            const int64_t nmv = s.C == 1 ? 1 : s.C;
            for (const char *which : {"dm", "ds", "dms"}) {
                snprintf(what, sizeof what, "quantize %s [%lld,%lld] y+%d", which, (long long)s.C, (long long)s.inner, off);
                CALL(what, which[1] == 's' ? quantize_ds(X(), Y(off), s.C, s.inner, MV(), nmv, 3.0f, 8, flag, nullptr)
                           : which[2]      ? quantize_dms(X(), Y(off), s.C, s.inner, MV(), nmv, MV(), 8, flag, nullptr)
                                           : quantize_dm(X(), Y(off), s.C, s.inner, MV(), nmv, MV(), 8, 1, nullptr));
            }
        }
    // min/max: reg, staged_mm, direct, split rows with the reducer block
    for (const Shape &s : {Shape{512, 576}, Shape{4096, 147}, Shape{64, 3}, Shape{4096, 147 * 4 + 1}, Shape{1, 2 << 20}, Shape{1, 32 << 20}, Shape{16, 1 << 20}})
        for (int off : {0, 1}) {
            snprintf(what, sizeof what, "minmax [%lld,%lld] x+%d", (long long)s.C, (long long)s.inner, off);
            CALL(what, minmax(X(off), s.C, s.inner, R(0), R(1), R(2), FP8Q_FOLD_CURRENT, 0.9, 1, R(3), ws_bytes(s.C, s.inner), nullptr));
        }
    // min/max + quantize: small fused (every EPL), reg, staged, flat fused, in place, direct fused
    const Shape fused[] = {{16, 9}, {16, 100}, {16, 147}, {16, 200}, {16, 400}, {512, 576}, {256, 1152}, {64, 4608}, {65536, 147}, {4096, 256},
                           {4096, 32}, {4096, 40}, {4096, 24}, {4096, 8}, {4096, 147}, {512, 577}, {2097152, 32}, {200000, 100}, {64, 9000}};
    for (const Shape &s : fused)
        for (float mb : widths) {
            snprintf(what, sizeof what, "minmax_quantize [%lld,%lld] M=%g", (long long)s.C, (long long)s.inner, mb);
            CALL(what, mmq(X(), Y(), s.C, s.inner, R(0), R(1), R(2), mb, 8, 1, nullptr));
        }
    CALL("minmax_quantize [4096,147] in place", mmq(X(), X(), 4096, 147, R(0), R(1), R(2), 3.0f, 8, 1, nullptr));
    CALL("minmax_quantize [4096,32] in place", mmq(X(), X(), 4096, 32, R(0), R(1), R(2), 3.0f, 8, 1, nullptr));
    CALL("minmax_quantize [4096,147] x,y+1", mmq(X(1), Y(1), 4096, 147, R(0), R(1), R(2), 3.0f, 8, 1, nullptr));
    // storage codes
    for (const Shape &s : {Shape{4096, 147}, Shape{4096, 32}, Shape{4096, 4}, Shape{2097152, 147}, Shape{64, 3}})
        for (float mb : widths) {
            snprintf(what, sizeof what, "encode / decode [%lld,%lld] M=%g", (long long)s.C, (long long)s.inner, mb);
            CALL(what, encode(X(), CODES(), s.C, s.inner, MV(), s.C, mb, 8, 1, nullptr));
            CALL(what, decode(CODES(), Y(), s.C, s.inner, MV(), s.C, mb, 8, 1, nullptr));
        }
    // multi-tensor plan: five tensors, the third misaligned, two formats
    const Shape ms[] = {{64, 147}, {128, 576}, {256, 1152}, {32, 27}, {100, 100}};
    for (int mode : {0, 3, 4}) {
        std::vector<fp8q_tensor_desc> d(5);
        float *mvs[5];
        for (int i = 0; i < 5; ++i) {
            const int off = i == 2 ? 1 : 0;
            d[i].x = mode == 4 ? reinterpret_cast<const float *>(CODES() + 0x1000000 * i) : R(i) + off;
            d[i].y = mode == 3 ? reinterpret_cast<float *>(CODES() + 0x1000000 * i) : R(5 + i) + off;
            d[i].maxval = mvs[i] = R(10 + i);
            d[i].C = ms[i].C, d[i].inner = ms[i].inner, d[i].n_maxval = ms[i].C;
            d[i].mbits = i & 1 ? 2.0f : 3.0f, d[i].n_bits = 8, d[i].sign_bits = 1;
        }
        snprintf(what, sizeof what, "multi plan mode %d", mode);
        CALL(what, mode == 0 ? multi_q(d.data(), 5, nullptr) : mode == 3 ? multi_e(d.data(), 5, nullptr) : multi_d(d.data(), 5, nullptr));
        if (mode == 0) CALL("multi minmax + quantize", multi_mmq(d.data(), mvs, 5, nullptr));
        if (mode == 3) CALL("multi minmax + encode", multi_mme(d.data(), mvs, 5, nullptr));
    }
    return rc;
}
