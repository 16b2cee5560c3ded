// Stand-alone check of the argument refusals of the sixteen launchers over the sparse digit list, the cluster table and the space points
// (csrc/pxd_clusters.hip, pxd_reco.hip, pxd_hits.hip, pxd_overlay.hip, pxd_match.hip, pxd_corr.hip, pxd_doublets.hip), for a sanitizer build of
// the host code:
//
//     hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Iinclude -Iiea-gan_amd/csrc \
//           iea-gan_amd/csrc/pxd_clusters.hip iea-gan_amd/csrc/pxd_reco.hip iea-gan_amd/csrc/pxd_hits.hip iea-gan_amd/csrc/pxd_overlay.hip \
//           iea-gan_amd/csrc/pxd_match.hip iea-gan_amd/csrc/pxd_corr.hip iea-gan_amd/csrc/pxd_doublets.hip tools/pxd_argcheck.cpp \
//           -o pxd_argcheck && ./pxd_argcheck
//
// Every call passes arguments a launcher must refuse before its first launch, so the program needs no GPU: it checks the return code and
// the error text, prints every refusal as it was received, and exits 0 when every refusal came.  Per launcher it walks what the Python host
// tests walk: every pointer NULL, every pointer misaligned, every scalar out of range.  What the launchers take from api.hip -- the error
// text and the profiling scope -- is restated below, since api.hip itself pulls in every other launcher of the library.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "common.h"
#include "ieagan_hip.h"
#include "ieagan_pxd_tracking.h"

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

static int failures = 0, refusals = 0;

static void expect(int rc, const char* text, const char* what) {
    const char* msg = ieagan_last_error();
    if (rc == 0 || std::strstr(msg, text) == nullptr) {
        std::printf("FAIL %s: rc = %d, error '%s', expected '%s'\n", what, rc, msg, text);
        ++failures;
    } else {
        std::printf("refused %-40s %s\n", what, msg);
        ++refusals;
    }
    g_err[0] = 0;
}

// A pointer argument of any type.
struct P {
    void* v;
    template <typename T> operator T*() const { return (T*)v; }
};
// The scalar arguments of all launchers; each takes what it has.
struct S {
    int N = 4, H = 8, W = 8, n_sensors = 2, K = 1, head_tail = 3, seed_cut = 0, charge_cut = 0, residual_bin = 10, E = 1;
    long capacity = 16, m_capacity = 16, a_digits = 8, b_digits = 8;
    int a_events = 2, b_events = 2;
    int tan_q12 = 1267, z0_sub = 320000;
    long doublet_capacity = 16;
};
// One pointer argument: the text of its refusal when it is NULL and when it is `off` bytes off (nullptr: no such refusal, a byte array).
struct Ptr {
    const char* name;
    const char* null_text;
    int off;
    const char* mis_text;
};
struct Scalar {
    void (*change)(S&);
    const char* text;
    const char* what;
};

alignas(64) static char buf[64 * 64];           // one 64-byte slot per pointer argument; no launcher reads it before it refuses

template <int NP, int NS, typename Call> static void walk(const char* fn, const Ptr (&ptrs)[NP], const Scalar (&scalars)[NS], Call call) {
    static_assert(NP <= 64, "one slot of buf per pointer");
    char what[96];
    P good[NP];
    for (int i = 0; i < NP; ++i) good[i].v = buf + 64 * i;
    for (const Scalar& c : scalars) {
        S s;
        c.change(s);
        std::snprintf(what, sizeof(what), "%s %s", fn, c.what);
        expect(call(good, s), c.text, what);
    }
    for (int i = 0; i < NP; ++i) {
        P p[NP];
        std::memcpy(p, good, sizeof(good));
        if (ptrs[i].null_text) {
            p[i].v = nullptr;
            std::snprintf(what, sizeof(what), "%s %s NULL", fn, ptrs[i].name);
            expect(call(p, S()), ptrs[i].null_text, what);
        }
        if (ptrs[i].mis_text) {
            p[i].v = (char*)good[i].v + ptrs[i].off;
            std::snprintf(what, sizeof(what), "%s %s + %d", fn, ptrs[i].name, ptrs[i].off);
            expect(call(p, S()), ptrs[i].mis_text, what);
        }
    }
}

#define GEOMETRY                                                                                                                      \
    {[](S& s) { s.N = 0; }, "outside 1 .. 65535", "N = 0"}, {[](S& s) { s.N = 65536; }, "outside 1 .. 65535", "N = 65536"},            \
    {[](S& s) { s.H = 0; }, "bad image size", "H = 0"}, {[](S& s) { s.W = -1; }, "bad image size", "W = -1"},                          \
    {[](S& s) { s.N = 64, s.H = s.W = 8192; }, "does not fit the int32 flat index", "2^32 pixels"}
#define CLUSTER_CHARGE {[](S& s) { s.H = s.W = 4096; }, "does not fit the int32 cluster charge", "H * W * 255 = 2^32"}
#define WHOLE_EVENTS                                                                                                                  \
    {[](S& s) { s.n_sensors = 0; }, "not a multiple of n_sensors", "n_sensors = 0"},                                                  \
    {[](S& s) { s.n_sensors = 3; }, "N = 4 is not a multiple of n_sensors = 3", "n_sensors = 3"}
#define CAPACITY {[](S& s) { s.capacity = -1; }, "capacity = -1 is negative", "capacity < 0"}

static void clusters() {
    const char *in = "index / charge is NULL with capacity 16", *out = "an output table is NULL with capacity 16",
               *al = "an int32 array is not 4-byte aligned", *ct = "counts / total is NULL or not 4-byte aligned", *sc = "scratch (";
    const Ptr ptrs[] = {{"index", in, 2, al},  {"charge", in, 0, nullptr}, {"digit_total", "digit_total is NULL or misaligned", 2, "digit_total is NULL or misaligned"},
                        {"label", out, 2, al}, {"first", out, 1, al},      {"size", out, 2, al},   {"ccharge", out, 3, al}, {"seed", out, 0, nullptr},
                        {"size_u", out, 2, al}, {"size_v", out, 2, al},    {"counts", ct, 2, ct},  {"total", ct, 2, ct},    {"scratch", sc, 2, sc}};
    const Scalar scalars[] = {GEOMETRY, CLUSTER_CHARGE, CAPACITY};
    walk("pxd_clusters", ptrs, scalars, [](const P* p, const S& s) {
        return ieagan_pxd_clusters(p[0], p[1], p[2], s.N, s.H, s.W, s.capacity, p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], nullptr);
    });
    const char *tb = "a cluster table is NULL with capacity 16", *tt = "cluster_total / digit_total is NULL or misaligned",
               *to = "tables / overflow is NULL or not 8-byte aligned";
    const Ptr sptrs[] = {{"first", tb, 0, nullptr},  {"size", tb, 0, nullptr},   {"ccharge", tb, 0, nullptr}, {"seed", tb, 0, nullptr},
                         {"size_u", tb, 0, nullptr}, {"size_v", tb, 0, nullptr}, {"cluster_total", tt, 2, tt}, {"digit_total", tt, 2, tt},
                         {"tables", to, 4, to},      {"overflow", to, 4, to}};
    const Scalar sscalars[] = {GEOMETRY, WHOLE_EVENTS, CAPACITY};
    walk("pxd_cluster_stats", sptrs, sscalars, [](const P* p, const S& s) {
        return ieagan_pxd_cluster_stats(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], s.N, s.H, s.W, s.n_sensors, s.capacity, p[8], p[9], nullptr);
    });
}

static void reco() {
    const char *in = "index / charge / label is NULL with capacity 16", *tb = "a cluster table is NULL with capacity 16",
               *out = "an output array is NULL with capacity 16", *al = "an int32 / fp32 array is not 4-byte aligned",
               *tt = "digit_total / cluster_total is NULL or misaligned", *m8 = "mu / mv is not 8-byte aligned",
               *ct = "counts / total is NULL or not 4-byte aligned", *sc = "scratch (";
    const Ptr ptrs[] = {{"index", in, 2, al},   {"charge", in, 0, nullptr}, {"label", in, 2, al},     {"digit_total", tt, 2, tt}, {"first", tb, 2, al},
                        {"ccharge", tb, 2, al}, {"seed", tb, 0, nullptr},   {"cluster_total", tt, 1, tt}, {"mu", out, 4, m8},     {"mv", out, 4, m8},
                        {"cluster", out, 2, al}, {"u", out, 2, al},         {"v", out, 1, al},        {"counts", ct, 2, ct},      {"total", ct, 2, ct},
                        {"scratch", sc, 2, sc}};
    const Scalar scalars[] = {GEOMETRY, CLUSTER_CHARGE, CAPACITY, {[](S& s) { s.seed_cut = -1; }, "seed_cut = -1 / charge_cut = 0 is negative", "seed_cut < 0"},
                              {[](S& s) { s.charge_cut = -5; }, "charge_cut = -5 is negative", "charge_cut < 0"}};
    walk("pxd_cluster_positions", ptrs, scalars, [](const P* p, const S& s) {
        return ieagan_pxd_cluster_positions(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], s.N, s.H, s.W, s.capacity, s.seed_cut, s.charge_cut, p[8],
                                            p[9], p[10], p[11], p[12], p[13], p[14], p[15], nullptr);
    });
    const char *ar = "cluster / first / ccharge / mu / mv is NULL with capacity 16", *a4 = "an int32 array is not 4-byte aligned",
               *t3 = "accepted_total / cluster_total / digit_total is NULL or misaligned", *o8 = "count / charge / overflow is NULL or not 8-byte aligned";
    const Ptr mptrs[] = {{"cluster", ar, 2, a4}, {"accepted_total", t3, 2, t3}, {"first", ar, 2, a4},       {"ccharge", ar, 2, a4}, {"mu", ar, 4, m8},
                         {"mv", ar, 4, m8},      {"cluster_total", t3, 2, t3},  {"digit_total", t3, 2, t3}, {"count", o8, 4, o8},   {"charge", o8, 4, o8},
                         {"overflow", o8, 4, o8}};
    const Scalar mscalars[] = {GEOMETRY, CLUSTER_CHARGE, WHOLE_EVENTS, CAPACITY};
    walk("pxd_cluster_maps", mptrs, mscalars, [](const P* p, const S& s) {
        return ieagan_pxd_cluster_maps(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], s.N, s.H, s.W, s.n_sensors, s.capacity, p[8], p[9], p[10], nullptr);
    });
}

static void hits() {
    const char *in = "index / charge / label is NULL with capacity 16", *tb = "a cluster table or the accepted list is NULL with capacity 16",
               *out = "an output array is NULL with capacity 16", *al = "an int32 / fp32 array is not 4-byte aligned",
               *tt = "digit_total / cluster_total / accepted_total is NULL or misaligned", *ge = "a geometry table is NULL or not 4-byte aligned",
               *p8 = "pu / pv is not 8-byte aligned";
    const Ptr ptrs[] = {{"index", in, 2, al},   {"charge", in, 0, nullptr}, {"label", in, 2, al},  {"digit_total", tt, 2, tt}, {"first", tb, 2, al},
                        {"ccharge", tb, 2, al}, {"size_u", tb, 2, al},      {"size_v", tb, 2, al}, {"cluster_total", tt, 2, tt}, {"cluster", tb, 2, al},
                        {"accepted_total", tt, 2, tt}, {"u_x2", ge, 2, ge}, {"u_pitch", ge, 2, ge}, {"v_x2", ge, 1, ge},       {"v_pitch", ge, 2, ge},
                        {"kind", ge, 2, ge},    {"pu", out, 4, p8},         {"pv", out, 4, p8},    {"v_start", out, 2, al},    {"qh_u", out, 2, al},
                        {"qt_u", out, 2, al},   {"qh_v", out, 2, al},       {"qt_v", out, 2, al},  {"u", out, 1, al},          {"v", out, 2, al},
                        {"flags", out, 0, nullptr}};
    const Scalar scalars[] = {GEOMETRY, CLUSTER_CHARGE, WHOLE_EVENTS, CAPACITY, {[](S& s) { s.K = 0; }, "K = 0 sensor types", "K = 0"},
                              {[](S& s) { s.head_tail = 1; }, "head_tail = 1 is neither", "head_tail = 1"},
                              {[](S& s) { s.head_tail = 2; }, "head_tail = 2 is neither", "head_tail = 2"},
                              {[](S& s) { s.head_tail = -3; }, "head_tail = -3 is neither", "head_tail = -3"}};
    walk("pxd_hits", ptrs, scalars, [](const P* p, const S& s) {
        return ieagan_pxd_hits(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13], p[14], p[15], s.N, s.H, s.W,
                               s.n_sensors, s.K, s.capacity, s.head_tail, p[16], p[17], p[18], p[19], p[20], p[21], p[22], p[23], p[24], p[25],
                               (int*)nullptr, nullptr);
    });
}

static void overlay() {
    const char *oo = "out_offsets is NULL or not 8-byte aligned", *sc = "scratch (";
    const Ptr ptrs[] = {{"a_pos", "a_pos / a_charge is NULL with digits 8", 2, "a_pos is not 4-byte aligned"},
                        {"a_charge", "a_pos / a_charge is NULL with digits 8", 0, nullptr},
                        {"a_offsets", "a_offsets is NULL with events 2", 4, "a_offsets is not 8-byte aligned"},
                        {"a_ids", "a_ids is NULL or misaligned", 1, "a_ids is NULL or misaligned"},
                        {"b_pos", "b_pos / b_charge is NULL with digits 8", 2, "b_pos is not 4-byte aligned"},
                        {"b_charge", "b_pos / b_charge is NULL with digits 8", 0, nullptr},
                        {"b_offsets", "b_offsets is NULL with events 2", 4, "b_offsets is not 8-byte aligned"},
                        {"b_ids", "b_ids is NULL or misaligned", 1, "b_ids is NULL or misaligned"},
                        {"out_pos", "out_pos / out_charge is NULL with capacity 16", 2, "out_pos is not 4-byte aligned"},
                        {"out_charge", "out_pos / out_charge is NULL with capacity 16", 0, nullptr},
                        {"out_offsets", oo, 4, oo},
                        {"scratch", sc, 2, sc}};
    // the geometry of a store is (S, H, W): S sensors an event, passed where the other launchers take N
    const Scalar scalars[] = {{[](S& s) { s.E = 0; }, "E = 0 pairs outside 1 .. 65535", "E = 0"}, {[](S& s) { s.E = 65536; }, "outside 1 .. 65535", "E = 65536"},
                              {[](S& s) { s.N = 0; }, "outside 1 .. 65535", "S = 0"}, {[](S& s) { s.H = 0; }, "bad image size", "H = 0"},
                              {[](S& s) { s.N = 64, s.H = s.W = 8192; }, "does not fit the int32 flat index", "2^32 pixels"}, CAPACITY,
                              {[](S& s) { s.a_digits = -1; }, "a_digits = -1 / a_events = 2 is negative", "a_digits < 0"},
                              {[](S& s) { s.a_events = -1; }, "a_events = -1 is negative", "a_events < 0"},
                              {[](S& s) { s.b_digits = -1; }, "b_digits = -1 / b_events = 2 is negative", "b_digits < 0"},
                              {[](S& s) { s.b_events = -1; }, "b_events = -1 is negative", "b_events < 0"}};
    walk("pxd_event_overlay", ptrs, scalars, [](const P* p, const S& s) {
        return ieagan_pxd_event_overlay(p[0], p[1], p[2], s.a_digits, s.a_events, p[3], p[4], p[5], p[6], s.b_digits, s.b_events, p[7], s.E, s.N, s.H, s.W,
                                        s.capacity, p[8], p[9], p[10], p[11], nullptr);
    });
}

static void match() {
    const char *st = "a total of the signal side is NULL or misaligned", *sa = "an array of the signal side is NULL with capacity 16",
               *s4 = "an int32 / fp32 array of the signal side is not 4-byte aligned", *mt = "a total of the mixed side is NULL or misaligned",
               *ma = "an array of the mixed side is NULL with capacity 16", *m4 = "an int32 / fp32 array of the mixed side is not 4-byte aligned",
               *cf = "s_charge / flags is NULL with capacity 16", *sc = "scratch (";
    const Ptr ptrs[] = {{"s_index", sa, 2, s4}, {"s_charge", cf, 0, nullptr}, {"s_label", sa, 2, s4}, {"s_digit_total", st, 2, st}, {"s_size", sa, 2, s4},
                        {"s_ccharge", sa, 2, s4}, {"s_cluster_total", st, 2, st}, {"s_cluster", sa, 2, s4}, {"s_accepted_total", st, 2, st},
                        {"s_u", sa, 2, s4}, {"s_v", sa, 1, s4}, {"m_index", ma, 2, m4}, {"m_label", ma, 2, m4}, {"m_digit_total", mt, 2, mt},
                        {"m_size", ma, 2, m4}, {"m_ccharge", ma, 2, m4}, {"m_cluster_total", mt, 2, mt}, {"m_cluster", ma, 2, m4},
                        {"m_accepted_total", mt, 2, mt}, {"m_u", ma, 2, m4}, {"m_v", ma, 3, m4}, {"found", sa, 2, s4}, {"lo", sa, 2, s4}, {"hi", sa, 2, s4},
                        {"signal_size", ma, 2, m4}, {"signal_charge", ma, 2, m4}, {"n_signal", ma, 2, m4}, {"mixed_hit", sa, 2, s4},
                        {"flags", cf, 0, nullptr}, {"du", sa, 2, s4}, {"dv", sa, 2, s4}, {"scratch", sc, 2, sc}};
    const Scalar scalars[] = {GEOMETRY, {[](S& s) { s.capacity = -1; }, "signal_capacity = -1 is negative", "s_capacity < 0"},
                              {[](S& s) { s.m_capacity = -1; }, "mixed_capacity = -1 is negative", "m_capacity < 0"}};
    walk("pxd_match", ptrs, scalars, [](const P* p, const S& s) {
        return ieagan_pxd_match(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13], p[14], p[15], p[16], p[17], p[18],
                                p[19], p[20], s.N, s.H, s.W, s.capacity, s.m_capacity, p[21], p[22], p[23], p[24], p[25], p[26], p[27], p[28], p[29],
                                p[30], p[31], nullptr);
    });
    const char *fl = "flags is NULL with capacity 16", *to = "table / overflow is NULL or not 8-byte aligned";
    const Ptr sptrs[] = {{"s_cluster", sa, 2, s4}, {"s_accepted_total", st, 2, st}, {"s_first", sa, 2, s4}, {"s_cluster_total", st, 2, st},
                         {"s_digit_total", st, 2, st}, {"s_u", sa, 2, s4}, {"s_v", sa, 2, s4}, {"m_ccharge", ma, 2, m4}, {"m_cluster_total", mt, 2, mt},
                         {"m_accepted_total", mt, 2, mt}, {"m_digit_total", mt, 2, mt}, {"m_u", ma, 2, m4}, {"m_v", ma, 2, m4}, {"lo", sa, 2, s4},
                         {"signal_charge", ma, 2, m4}, {"mixed_hit", sa, 2, s4}, {"flags", fl, 0, nullptr}, {"table", to, 4, to}, {"overflow", to, 4, to}};
    const Scalar sscalars[] = {GEOMETRY, WHOLE_EVENTS, {[](S& s) { s.residual_bin = 0; }, "residual_bin = 0 is not >= 1", "residual_bin = 0"},
                               {[](S& s) { s.residual_bin = -5; }, "residual_bin = -5 is not >= 1", "residual_bin = -5"},
                               {[](S& s) { s.capacity = -1; }, "signal_capacity = -1 is negative", "s_capacity < 0"},
                               {[](S& s) { s.m_capacity = -1; }, "mixed_capacity = -1 is negative", "m_capacity < 0"}};
    walk("pxd_match_stats", sptrs, sscalars, [](const P* p, const S& s) {
        return ieagan_pxd_match_stats(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], p[13], p[14], p[15], p[16], s.N,
                                      s.H, s.W, s.n_sensors, s.capacity, s.m_capacity, s.residual_bin, p[17], p[18], nullptr);
    });
}

// The three launchers of pxd_corr.hip, call by call.
static void corr() {
    alignas(16) static long long cbuf[64];
    int* i32 = (int*)cbuf;
    int* total = (int*)(cbuf + 8);
    int* x = (int*)(cbuf + 16);
    unsigned long long* overflow = (unsigned long long*)(cbuf + 32);
    long long* gram = cbuf + 40;
    long long* sum = cbuf + 48;
    char* bytes = (char*)cbuf;
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
}

// The three launchers of pxd_doublets.hip (include/ieagan_pxd_tracking.h) and the scratch size.
static void tracking() {
    const char *tt = "accepted_total / cluster_total is NULL or misaligned", *pl = "a placement table is NULL or not 4-byte aligned",
               *co = "counts / offsets is NULL or not 4-byte aligned", *in = "cluster / first / u / v is NULL with capacity 16",
               *out = "an output array is NULL with capacity 16", *al = "an int32 / fp32 array is not 4-byte aligned";
#define SHAPE                                                                                                                         \
    {[](S& s) { s.N = 0; }, "N = 0 outside 1 .. 65535", "N = 0"}, {[](S& s) { s.N = 65536; }, "outside 1 .. 65535", "N = 65536"},      \
    {[](S& s) { s.n_sensors = 0; }, "n_sensors = 0 outside 1 .. 255", "n_sensors = 0"},                                               \
    {[](S& s) { s.N = 512, s.n_sensors = 256; }, "n_sensors = 256 outside 1 .. 255", "n_sensors = 256"},                              \
    {[](S& s) { s.n_sensors = 3; }, "N = 4 is not a multiple of n_sensors = 3", "n_sensors = 3"}, CAPACITY
    const Ptr ptrs[] = {{"cluster", in, 2, al}, {"accepted_total", tt, 2, tt}, {"first", in, 2, al}, {"cluster_total", tt, 2, tt}, {"counts", co, 2, co},
                        {"u", in, 2, al},       {"v", in, 1, al},              {"origin", pl, 2, pl}, {"u_axis", pl, 2, pl},       {"v_axis", pl, 1, pl},
                        {"layer", pl, 2, pl},   {"x", out, 2, al},             {"y", out, 2, al},     {"z", out, 2, al},           {"r", out, 3, al},
                        {"sensor", out, 2, al}, {"role", out, 0, nullptr},     {"offsets", co, 2, co}};
    const Scalar scalars[] = {SHAPE, {[](S& s) { s.H = 0; }, "bad image size", "H = 0"}, {[](S& s) { s.W = -1; }, "bad image size", "W = -1"},
                              {[](S& s) { s.N = 64, s.n_sensors = 64, s.H = s.W = 8192; }, "does not fit the int32 flat index", "2^32 pixels"}};
    walk("pxd_space_points", ptrs, scalars, [](const P* p, const S& s) {
        return ieagan_pxd_space_points(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], s.N, s.H, s.W, s.n_sensors, s.capacity, p[11],
                                       p[12], p[13], p[14], p[15], p[16], p[17], nullptr);
    });
    const char *sp = "a space-point array is NULL with capacity 16", *a4 = "an int32 array is not 4-byte aligned",
               *oe = "offsets / event_doublets / pair_doublets / total is NULL or not 4-byte aligned", *io = "inner / outer is NULL with doublet_capacity 16",
               *sc = "scratch (", *at = "accepted_total is NULL or misaligned";
    const Ptr dptrs[] = {{"x", sp, 2, a4},      {"y", sp, 2, a4},       {"z", sp, 2, a4},           {"r", sp, 2, a4},  {"sensor", sp, 1, a4},
                         {"role", sp, 0, nullptr}, {"offsets", oe, 2, oe}, {"accepted_total", at, 2, at}, {"pairs", "pairs is NULL", 0, nullptr},
                         {"partners", "partners is NULL with capacity 16", 2, a4}, {"event_doublets", oe, 2, oe}, {"pair_doublets", oe, 2, oe}, {"total", oe, 3, oe},
                         {"inner", io, 2, a4},  {"outer", io, 2, a4},   {"scratch", sc, 2, sc}};
    const Scalar dscalars[] = {SHAPE,
                               {[](S& s) { s.doublet_capacity = -1; }, "doublet_capacity = -1 is negative", "doublet_capacity < 0"},
                               {[](S& s) { s.tan_q12 = 0; }, "tan_q12 = 0 outside 1 .. 32768", "tan_q12 = 0"},
                               {[](S& s) { s.tan_q12 = 32769; }, "tan_q12 = 32769 outside", "tan_q12 = 32769"},
                               {[](S& s) { s.tan_q12 = -2147483647 - 1; }, "outside 1 .. 32768", "tan_q12 = INT_MIN"},
                               {[](S& s) { s.z0_sub = -1; }, "z0_sub = -1 outside", "z0_sub = -1"},
                               {[](S& s) { s.z0_sub = 1 << 23; }, "z0_sub = 8388608 outside 0 .. 2^23 - 1", "z0_sub = 2^23"}};
    walk("pxd_doublets", dptrs, dscalars, [](const P* p, const S& s) {
        return ieagan_pxd_doublets(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], s.N, s.n_sensors, s.capacity, s.tan_q12, s.z0_sub,
                                   s.doublet_capacity, p[9], p[10], p[11], p[12], p[13], p[14], p[15], nullptr);
    });
    const char *t2 = "accepted_total / digit_total is NULL or misaligned", *ol = "offsets / layer / event_doublets / pair_doublets is NULL or not 4-byte aligned",
               *to = "tables / overflow is NULL or not 8-byte aligned", *rp = "role / partners is NULL with capacity 16";
    const Ptr sptrs[] = {{"role", rp, 0, nullptr}, {"offsets", ol, 2, ol},        {"accepted_total", t2, 2, t2}, {"digit_total", t2, 2, t2}, {"layer", ol, 2, ol},
                         {"partners", rp, 2, "partners is not 4-byte aligned"}, {"event_doublets", ol, 1, ol}, {"pair_doublets", ol, 2, ol},
                         {"tables", to, 4, to},    {"overflow", to, 4, to}};
    const Scalar sscalars[] = {SHAPE};
    walk("pxd_doublet_stats", sptrs, sscalars, [](const P* p, const S& s) {
        return ieagan_pxd_doublet_stats(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], s.N, s.n_sensors, s.capacity, p[8], p[9], nullptr);
    });
#undef SHAPE
    if (ieagan_pxd_doublets_scratch(40, 40, 480000) != 4 * (480000 / 256 + 1 + 1) || ieagan_pxd_doublets_scratch(0, 4, 16) != 0 ||
        ieagan_pxd_doublets_scratch(4, 0, 16) != 0 || ieagan_pxd_doublets_scratch(4, 2, -1) != 0) {
        std::printf("FAIL pxd_doublets_scratch\n");
        ++failures;
    }
}

int main() {
    clusters();
    reco();
    hits();
    overlay();
    match();
    corr();
    tracking();
    std::printf("%s: %d refusal(s) received, %d missing\n", failures ? "FAILED" : "ok", refusals, failures);
    return failures ? 1 : 0;
}
