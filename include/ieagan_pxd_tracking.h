/* C ABI of libieagan_hip.so, second header: PXD space points and inner / outer-layer hit doublets (csrc/pxd_doublets.hip).
 *
 * The conventions are those of ieagan_hip.h, which this header includes: `extern "C"`, plain pointers and sizes, the hipStream_t last (as
 * void*), no allocation, no synchronisation, no copy; 0 on success, negative on error, the text through ieagan_last_error().  The entry
 * points live in the same library and IEAGAN_ABI_VERSION is unchanged: nothing declared in ieagan_hip.h changed.  They stand in a header of
 * their own because ieagan_hip.h is the interface of the train step and of the per-sensor detector chain, whose number of entry points is
 * pinned by the tests of that chain; the relational products -- anything that needs to know where a sensor sits in space -- start here.
 *
 * Units: sub-units of 1 / 16 geometry unit (pxd.PXDGeometry.unit_mm / 16).  A placement is data, per sensor s of n_sensors (1 .. 255):
 *   origin [S * 3] int32   the sensor centre, sub-units         u_axis / v_axis [S * 3] int32   the global directions of local u (rows) and
 *   layer  [S] int32       0 inner, 1 outer, else ignored                                       v (columns), Q30: |a| <= 2^30
 *   pairs  [S * S] uint8   a doublet of inner sensor i and outer sensor o counts only when pairs[i * S + o] != 0
 * The host (pxd.PXDPlacement) keeps every corner of every sensor below 2^23 sub-units; that bound keeps every product below inside int64. */
#ifndef IEAGAN_PXD_TRACKING_H
#define IEAGAN_PXD_TRACKING_H
#include "ieagan_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The hits of one ieagan_pxd_hits result (cluster / accepted_total / counts of ieagan_pxd_cluster_positions, first / cluster_total of
 * ieagan_pxd_clusters, u / v fp32 in geometry units) in the global frame.  Per hit row a below min(*accepted_total, *cluster_total, capacity):
 *   s = (first[cluster[a]] / (H * W)) % n_sensors;  lu = (int)rintf(u[a] * 16.0f), lv likewise (exact multiply, round to nearest even)
 *   x / y / z [capacity] int32   X_c = origin[s][c] + ((u_axis[s][c] * lu + v_axis[s][c] * lv + 2^29) >> 30), int64 arithmetic shift
 *   r [capacity] int32           floor(sqrt(x^2 + y^2)) exactly
 *   sensor [capacity] int32      s;  role [capacity] int8: layer[s] when it is 0 or 1, else -1
 *   offsets [N + 1] int32        the exclusive prefix of counts [N]: hits are stored image by image, the rows of image n are
 *                                [offsets[n], offsets[n + 1])
 * A cluster row outside the table gives a point at the origin with sensor -1 and role -1.  Two launches whose shapes depend on (N, capacity)
 * alone (graph-capturable; capacity 0: the arrays may be NULL). */
int ieagan_pxd_space_points(const int* cluster, const int* accepted_total, const int* first, const int* cluster_total, const int* counts,
                            const float* u, const float* v, const int* origin, const int* u_axis, const int* v_axis, const int* layer, int N,
                            int H, int W, int n_sensors, long capacity, int* x, int* y, int* z, int* r, int* sensor, signed char* role,
                            int* offsets, void* stream);

/* Doublets of one ieagan_pxd_space_points result.  Hit a with role 0 and hit b with role 1 of the same event (the rows
 * [offsets[e * n_sensors], offsets[(e + 1) * n_sensors]) of event e, E = N / n_sensors) form a doublet iff, in int64,
 *   pairs[sensor[a] * n_sensors + sensor[b]] != 0
 *   dot = x_a x_b + y_a y_b > 0  and  |x_a y_b - y_a x_b| << 12 <= tan_q12 * dot              1 <= tan_q12 <= 32768
 *   r_b > r_a  and  |z_a r_b - z_b r_a| <= z0_sub * (r_b - r_a)                                 0 <= z0_sub < 2^23
 *   partners [capacity] int32        the doublets of hit row a; 0 for a row that is no inner hit (written for every row of an event)
 *   event_doublets [E] int32         the doublets of event e
 *   pair_doublets [S * S] int32      the doublets of (inner sensor, outer sensor)
 *   total [1] int32                  the doublets of the batch
 *   inner / outer [doublet_capacity] int32   the hit rows of the first min(total, doublet_capacity) doublets in ascending (inner, outer)
 * partners, event_doublets, pair_doublets and total are whole whatever doublet_capacity is.  Integer arithmetic and int32 atomics only: two calls write
 * the same bytes.  The accepted total is clipped to the capacity, every offset to [0, total], a sensor is compared with n_sensors before it
 * indexes pairs and a list position with doublet_capacity: inputs that break their contract give wrong numbers, never a wrong address.
 * Four launches whose shapes depend on (N, n_sensors, capacity) alone (graph-capturable).
 * scratch: ieagan_pxd_doublets_scratch(N, n_sensors, capacity) int32 words. */
long ieagan_pxd_doublets_scratch(int N, int n_sensors, long capacity);
int ieagan_pxd_doublets(const int* x, const int* y, const int* z, const int* r, const int* sensor, const signed char* role,
                        const int* offsets, const int* accepted_total, const unsigned char* pairs, int N, int n_sensors, long capacity,
                        int tan_q12, int z0_sub, long doublet_capacity, int* partners, int* event_doublets, int* pair_doublets, int* total,
                        int* inner, int* outer, int* scratch, void* stream);

/* Accumulates one ieagan_pxd_doublets result into tables int64 [5 + S * S + 64 + 251], S = n_sensors:
 *   [0 .. 4]                 events, inner hits, outer hits, doublets, sum over the events of n_in(e) * n_out(e)
 *   [5 .. 5 + S * S)         doublets per (inner sensor, outer sensor): pair_doublets
 *   then 64                  partners over the inner hits, bin min(partners, 63)
 *   then 251                 event_doublets over the events, the bins of ieagan_pxd_stats: d < 1 -> 0, d < 7 -> 1, else 2 + min(d - 7, 248)
 * overflow [1] int64: + 1 when *digit_total > capacity (hits of a truncated digit list).  The list inner / outer is not read: the statistics
 * do not depend on doublet_capacity.  One launch, 64-bit integer atomics. */
int ieagan_pxd_doublet_stats(const signed char* role, const int* offsets, const int* accepted_total,
                             const int* digit_total, const int* layer, const int* partners, const int* event_doublets,
                             const int* pair_doublets, int N, int n_sensors, long capacity, unsigned long long* tables,
                             unsigned long long* overflow, void* stream);

#ifdef __cplusplus
}
#endif
#endif
