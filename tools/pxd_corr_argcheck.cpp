// Stand-alone check of the argument refusals of the three launchers of csrc/pxd_corr.hip, for a sanitizer build of the host code:
//
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Iinclude -Iiea-gan_amd/csrc \
//           iea-gan_amd/csrc/pxd_corr.hip tools/pxd_corr_argcheck.cpp -o pxd_corr_argcheck && ./pxd_corr_argcheck
//
// Every call passes arguments a launcher must refuse before its first launch, so the program needs no GPU: it checks the return code and
// the error text, and exits 0 when every refusal came.  What the launchers take from api.hip -- the error text and the profiling scope --
// is restated below, since api.hip itself pulls in every other launcher of the library.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "common.h"
#include "ieagan_hip.h"

static char g_err[512] = "";

void ieagan_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* ieagan_last_error(void) { return g_err; }
ProfScope::ProfScope(const char*, double, double, hipStream_t, const char*, double) : active(false) {}
ProfScope::~ProfScope() {}

static int failures = 0;

static void expect(int rc, const char* text, const char* what) {
    const char* msg = ieagan_last_error();
    if (rc == 0 || std::strstr(msg, text) == nullptr) {
        std::printf("FAIL %s: rc = %d, error '%s', expected '%s'\n", what, rc, msg, text);
        ++failures;
    }
}

int main() {
    alignas(16) static long long buf[64];
    int* i32 = (int*)buf;
    int* total = (int*)(buf + 8);
    int* x = (int*)(buf + 16);
    unsigned long long* overflow = (unsigned long long*)(buf + 32);
    long long* gram = buf + 40;
    long long* sum = buf + 48;
    char* bytes = (char*)buf;
    const int N = 4, H = 8, W = 12, S = 2, RU = 2, RV = 3;
    const long cap = 16;

    expect(ieagan_pxd_region_counts(i32, total, 0, H, W, S, RU, RV, cap, x, overflow, nullptr), "outside 1 .. 65535", "N = 0");
    expect(ieagan_pxd_region_counts(i32, total, 65536, H, W, S, RU, RV, cap, x, overflow, nullptr), "outside 1 .. 65535", "N = 65536");
    expect(ieagan_pxd_region_counts(i32, total, N, 0, W, S, RU, RV, cap, x, overflow, nullptr), "bad image size", "H = 0");
    expect(ieagan_pxd_region_counts(i32, total, N, H, -1, S, RU, RV, cap, x, overflow, nullptr), "bad image size", "W = -1");
    expect(ieagan_pxd_region_counts(i32, total, 64, 8192, 8192, S, RU, RV, cap, x, overflow, nullptr), "does not fit the int32 flat index", "2^32 pixels");
    expect(ieagan_pxd_region_counts(i32, total, N, H, W, 0, RU, RV, cap, x, overflow, nullptr), "not a multiple of n_sensors", "n_sensors = 0");
    expect(ieagan_pxd_region_counts(i32, total, N, H, W, 3, RU, RV, cap, x, overflow, nullptr), "not a multiple of n_sensors", "n_sensors = 3");
    expect(ieagan_pxd_region_counts(i32, total, N, H, W, S, 0, RV, cap, x, overflow, nullptr), "regions 0 x 3 outside", "RU = 0");
    expect(ieagan_pxd_region_counts(i32, total, N, H, W, S, H + 1, RV, cap, x, overflow, nullptr), "regions 9 x 3 outside", "RU > H");
    expect(ieagan_pxd_region_counts(i32, total, N, H, W, S, RU, -2147483647 - 1, cap, x, overflow, nullptr), "outside", "RV = INT_MIN");
    expect(ieagan_pxd_region_counts(i32, total, N, H, W, S, RU, W + 1, cap, x, overflow, nullptr), "regions 2 x 13 outside", "RV > W");
    expect(ieagan_pxd_region_counts(i32, total, 1024, 4096, 4, 1024, 4096, 4, cap, x, overflow, nullptr), "columns exceed 1024", "R = 2^24");
    expect(ieagan_pxd_region_counts(i32, total, 40, 250, 768, 40, 2, 13, cap, x, overflow, nullptr), "columns exceed 1024", "R = 1040");
    expect(ieagan_pxd_region_counts(i32, total, N, H, W, S, RU, RV, -1, x, overflow, nullptr), "capacity = -1 is negative", "capacity < 0");
    expect(ieagan_pxd_region_counts(i32, nullptr, N, H, W, S, RU, RV, cap, x, overflow, nullptr), "digit_total is NULL", "digit_total NULL");
    expect(ieagan_pxd_region_counts(i32, (int*)(bytes + 2), N, H, W, S, RU, RV, cap, x, overflow, nullptr), "digit_total is NULL or misaligned", "digit_total + 2");
    expect(ieagan_pxd_region_counts(nullptr, total, N, H, W, S, RU, RV, cap, x, overflow, nullptr), "index is NULL with capacity 16", "index NULL");
    expect(ieagan_pxd_region_counts((int*)(bytes + 1), total, N, H, W, S, RU, RV, cap, x, overflow, nullptr), "not 4-byte aligned", "index + 1");
    expect(ieagan_pxd_region_counts(i32, total, N, H, W, S, RU, RV, cap, nullptr, overflow, nullptr), "x is NULL", "x NULL");
    expect(ieagan_pxd_region_counts(i32, total, N, H, W, S, RU, RV, cap, (int*)(bytes + 3), overflow, nullptr), "x is NULL or not 4-byte aligned", "x + 3");
    expect(ieagan_pxd_region_counts(i32, total, N, H, W, S, RU, RV, cap, x, nullptr, nullptr), "overflow is NULL", "overflow NULL");
    expect(ieagan_pxd_region_counts(i32, total, N, H, W, S, RU, RV, cap, x, (unsigned long long*)(bytes + 4), nullptr), "not 8-byte aligned", "overflow + 4");

    expect(ieagan_pxd_gram(x, 0, 18, gram, sum, nullptr), "E = 0 outside", "gram E = 0");
    expect(ieagan_pxd_gram(x, 65536, 18, gram, sum, nullptr), "E = 65536 outside", "gram E = 65536");
    expect(ieagan_pxd_gram(x, -2147483647 - 1, 18, gram, sum, nullptr), "outside 1 .. 65535", "gram E = INT_MIN");
    expect(ieagan_pxd_gram(x, 7, 0, gram, sum, nullptr), "R = 0 outside", "gram R = 0");
    expect(ieagan_pxd_gram(x, 7, 1025, gram, sum, nullptr), "R = 1025 outside", "gram R = 1025");
    expect(ieagan_pxd_gram(nullptr, 7, 18, gram, sum, nullptr), "x is NULL", "gram x NULL");
    expect(ieagan_pxd_gram((int*)(bytes + 2), 7, 18, gram, sum, nullptr), "not 4-byte aligned", "gram x + 2");
    expect(ieagan_pxd_gram(x, 7, 18, nullptr, sum, nullptr), "gram / sum is NULL", "gram NULL");
    expect(ieagan_pxd_gram(x, 7, 18, gram, nullptr, nullptr), "gram / sum is NULL", "sum NULL");
    expect(ieagan_pxd_gram(x, 7, 18, (long long*)(bytes + 4), sum, nullptr), "not 8-byte aligned", "gram + 4");
    expect(ieagan_pxd_gram(x, 7, 18, gram, (long long*)(bytes + 4), nullptr), "not 8-byte aligned", "sum + 4");

    expect(ieagan_pxd_ranks(x, 0, 18, i32, nullptr), "E = 0 outside", "ranks E = 0");
    expect(ieagan_pxd_ranks(x, 65536, 18, i32, nullptr), "E = 65536 outside", "ranks E = 65536");
    expect(ieagan_pxd_ranks(x, 7, 0, i32, nullptr), "R = 0 outside", "ranks R = 0");
    expect(ieagan_pxd_ranks(x, 7, 2147483647, i32, nullptr), "outside 1 .. 1024", "ranks R = INT_MAX");
    expect(ieagan_pxd_ranks(nullptr, 7, 18, i32, nullptr), "x is NULL", "ranks x NULL");
    expect(ieagan_pxd_ranks(x, 7, 18, nullptr, nullptr), "rank2 is NULL", "rank2 NULL");
    expect(ieagan_pxd_ranks(x, 7, 18, (int*)(bytes + 2), nullptr), "not 4-byte aligned", "rank2 + 2");
    expect(ieagan_pxd_ranks(x, 7, 18, x, nullptr), "rank2 must not be x", "rank2 == x");

    std::printf("%s: %d refusal(s) missing\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
