/*
 * cwipc_util_amd/hip_ext.h -- device-side extensions of the MI355X libcwipc_util.
 *
 * None of these symbols exist in the reference; they expose what a GPU-resident
 * pipeline needs on top of the drop-in C-ABI of cwipc_util/api.h: device
 * selection, explicit residency control, zero-copy access to the SoA planes
 * (so torch.distributed / RCCL can move them), two filters whose reference
 * implementation is Python-side, and per-kernel timing for bench.py.
 * Plain C: pointers and sizes only, no torch types.
 */
#ifndef CWIPC_UTIL_AMD_HIP_EXT_H
#define CWIPC_UTIL_AMD_HIP_EXT_H

#include "cwipc_util/api.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- device management ---- */
_CWIPC_UTIL_EXPORT int cwipc_hip_device_count(void);          /* 0 when no GPU is visible */
_CWIPC_UTIL_EXPORT int cwipc_hip_set_device(int device);      /* process-wide device for all later calls; 0 ok, -1 error */
_CWIPC_UTIL_EXPORT int cwipc_hip_get_device(void);
_CWIPC_UTIL_EXPORT const char *cwipc_hip_last_error(void);    /* thread-local text of the last HIP failure ("" if none) */
_CWIPC_UTIL_EXPORT void cwipc_hip_synchronize(void);          /* wait for the calling thread's stream */
_CWIPC_UTIL_EXPORT size_t cwipc_hip_pool_bytes(void);         /* bytes currently held by the device memory pool */
_CWIPC_UTIL_EXPORT size_t cwipc_hip_workspace_bytes(void);    /* device bytes held by the voxel filter's workspaces (leaf grids; two per thread that downsamples) */
_CWIPC_UTIL_EXPORT void cwipc_hip_pool_trim(void);            /* return cached device memory to the driver */
_CWIPC_UTIL_EXPORT size_t cwipc_hip_workspace_trim(void);     /* give back the voxel workspaces that ended threads left for the next ones (at most 8); returns how many */

/* ---- page-locked host buffers of the caller (round 4) ----
 * The copy path of the reference (src/cwipc_util.cpp:329-354 from_points, :226-250 copy_uncompressed) moves bytes between the
 * caller's buffer and a buffer the cloud owns.  Here the owned copy lives in HBM, and a buffer the DMA engines cannot reach costs
 * one more copy on the host on the way.  A caller that keeps its point buffers in page-locked memory -- allocated here, or its own
 * memory registered once (a numpy array that is reused frame after frame) -- skips it: cwipc_from_points / cwipc_from_packet read
 * such a buffer straight from the device (and have finished reading when they return, as the reference's copy has),
 * cwipc_pointcloud_copy_uncompressed / copy_packet into one are written by the DMA engine directly.  Nothing else changes. */
_CWIPC_UTIL_EXPORT void *cwipc_hip_host_alloc(size_t bytes);                 /* NULL without a GPU or memory */
_CWIPC_UTIL_EXPORT void cwipc_hip_host_free(void *ptr);
_CWIPC_UTIL_EXPORT int cwipc_hip_host_register(void *ptr, size_t bytes);     /* 0 ok; the memory stays the caller's */
_CWIPC_UTIL_EXPORT int cwipc_hip_host_unregister(void *ptr);

/* ---- residency ----
 * A cloud made by cwipc_from_points lives in host memory until a filter needs
 * it; filter results live in HBM (SoA planes x,y,z:f32[n], rgbt:u32[n] with
 * r | g<<8 | b<<16 | tile<<24) until a host accessor needs them. */
_CWIPC_UTIL_EXPORT int cwipc_hip_upload(cwipc_pointcloud *pc);            /* make the SoA copy now; 0 ok */
_CWIPC_UTIL_EXPORT int cwipc_hip_drop_host_copy(cwipc_pointcloud *pc);    /* free the host AoS copy (device copy must exist) */
_CWIPC_UTIL_EXPORT int cwipc_hip_is_device_resident(cwipc_pointcloud *pc);
_CWIPC_UTIL_EXPORT int cwipc_hip_device_planes(cwipc_pointcloud *pc, const float **x, const float **y, const float **z,
                                               const uint32_t **rgbt, size_t *npoint);
/* Interleave the planes into a DEVICE buffer of npoint*16 bytes (cwipc_point records). Returns npoint or -1. */
_CWIPC_UTIL_EXPORT long cwipc_hip_copy_device_aos(cwipc_pointcloud *pc, void *dev_points, size_t size);
/* New cloud from cwipc_point records that already are in device memory. */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_from_device_aos(const void *dev_points, size_t npoint, uint64_t timestamp, float cellsize);
/* The same from the receive buffer of an all-gather (the multi-GPU join, reference cwipc_join folded over the tiles,
   src/cwipc_filters.cpp:388-418): nslots (<= 64) slots of slot_rows 16-byte rows each in device memory, the records of
   slot s in rows [header_rows, header_rows + counts[s]); the new cloud holds them in slot order.  counts is a host array. */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_from_device_slots(const void *dev_slots, int nslots, size_t slot_rows, size_t header_rows,
                                                                 const uint32_t *counts, uint64_t timestamp, float cellsize);
/* Both as steps of the CALLER's stream (hipStream_t; e.g. the stream its collectives are ordered on): no wait inside, the
   kernel runs behind what the stream holds and in front of what the caller enqueues next; the new cloud carries an event. */
_CWIPC_UTIL_EXPORT long cwipc_hip_copy_device_aos_on_stream(cwipc_pointcloud *pc, void *dev_points, size_t size, void *stream);
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_from_device_slots_on_stream(const void *dev_slots, int nslots, size_t slot_rows, size_t header_rows,
                                                                           const uint32_t *counts, uint64_t timestamp, float cellsize, void *stream);

/* ---- the multi-GPU join: one process per GPU, RCCL inside the library, one call per frame ----
 * Replaces the reference's in-process fold of cwipc_join over a frame's tiles (python/cwipc/net/source_synchronizer.py:175-188,
 * src/cwipc_filters.cpp:388-418) when the tiles live on different GPUs.  Bootstrap as with any RCCL communicator: one rank
 * asks for an id, the application hands its bytes to the other ranks (MPI, a socket, torch.distributed's store ...), every
 * rank creates its end on the device chosen with cwipc_hip_set_device.  With nranks > 1 the call REFUSES to start unless
 * HSA_ENABLE_IPC_MODE_LEGACY=0 is in the environment (this image's driver: RCCL's buffer hand-over between processes fails
 * without it, inside the first collective). */
#define CWIPC_HIP_COMM_ID_BYTES 128
typedef struct cwipc_hip_comm cwipc_hip_comm;
_CWIPC_UTIL_EXPORT int cwipc_hip_comm_unique_id(void *id /* CWIPC_HIP_COMM_ID_BYTES */, char **errorMessage);              /* 0 ok */
_CWIPC_UTIL_EXPORT cwipc_hip_comm *cwipc_hip_comm_create(const void *id, int rank, int nranks, char **errorMessage);       /* collective */
_CWIPC_UTIL_EXPORT void cwipc_hip_comm_free(cwipc_hip_comm *comm);
_CWIPC_UTIL_EXPORT int cwipc_hip_comm_rank(cwipc_hip_comm *comm);
_CWIPC_UTIL_EXPORT int cwipc_hip_comm_nranks(cwipc_hip_comm *comm);
/* Every rank calls this once per frame with its cloud (NULL: no tile this frame) and gets the fused cloud: the ranks' points in
 * rank order, timestamp and cellsize the minimum over the clouds that took part (src/cwipc_filters.cpp:411-414).  One
 * ncclAllGather of 32 bytes per rank, then one group of ncclSend/ncclRecv that moves the planes straight into the result; the
 * call returns when the group is enqueued (the result carries an event).  NULL on error (logged).  What a single rank finds
 * out on its own (no usable device, no memory for the fused cloud) travels in its record, so the others leave it out instead
 * of waiting for it; a rank whose tile is the whole frame gets its own planes back and still sends them to the others. */
#define CWIPC_HIP_JOIN_LOOPBACK 1   /* this rank's own part travels through RCCL too (send/recv to itself): exercises the exchange on one GPU */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_comm_join(cwipc_hip_comm *comm, cwipc_pointcloud *pc, int flags);
/* The same for a stream of frames: returns at once with a cloud that stands for the fused cloud of this frame; the exchange
 * itself (waiting for this rank's filter results, the record all-gather, the send/recv group) is done by a thread of the
 * communicator, frame after frame in the order of the calls, and the cloud settles when it is first used (count, a filter, a
 * copy; its timestamp and cellsize too: they are the minimum over the ranks).  Every rank submits every frame, in the same
 * order.  The argument may be freed as soon as the call returns.  A failed exchange shows as an empty cloud plus the logged
 * error.  cwipc_hip_comm_free waits for the frames still queued. */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_comm_submit(cwipc_hip_comm *comm, cwipc_pointcloud *pc, int flags);

/* Test hook, pure host code (works without a GPU): the plan rank `rank` of `nranks` follows for a frame whose gathered records are
 * `metas` (nranks x 8 uint32: count, has_cloud, cellsize bits, status [0 ok, 1 absent, 2 sends but cannot receive], ts_lo, ts_hi,
 * capacity, 0) -- the very function cwipc_hip_comm_join issues its ncclSend / ncclRecv from (csrc/exchange_plan.hpp).
 * summary[8] = total points, flags (1 too big, 2 no result on this rank, 4 result = this rank's input, 8 own part by copy kernel,
 * 16 some tile arrived, 32 the ranks meet a second time before payload moves, 64 this rank needs a result buffer), ts_min,
 * cellsize bits, this rank's displacement, number of sends, number of receives, 0; sends / recvs: cap x {peer, points, offset}.
 * Returns 0, -1 bad arguments, -2 cap too small. */
_CWIPC_UTIL_EXPORT int cwipc_hip_exchange_plan(int rank, int nranks, const uint32_t *metas, int loopback, uint64_t *summary,
                                               uint64_t *sends, uint64_t *recvs, int cap);

/* ---- the proxy's wire format as a packet codec (reference src/cwipc_proxy.cpp:179-216, include/cwipc_util/api.h:100-110) ----
 * A packet = the 24-byte cwipc_point_packetheader + dataCount bytes of cwipc_point records; the receiver's answer is the 8 bytes of
 * the timestamp.  No sockets here: the application moves the bytes.
 * cwipc_hip_proxy_packet: writes the packet of `pc` (magic 0 = CWIPC_POINT_PACKETHEADER_MAGIC); packet NULL: returns the size it
 * takes; returns the bytes written, 0 on error.  cwipc_hip_from_proxy_packet: the cloud of a packet (timestamp and cellsize from
 * the header); the C magic is always accepted, the reference's Python sender's (0x20210208, python/cwipc/util.py:346 -- the two
 * disagree upstream) only when accept_python_magic is set. */
_CWIPC_UTIL_EXPORT size_t cwipc_hip_proxy_packet(cwipc_pointcloud *pc, uint8_t *packet, size_t size, uint32_t magic);
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_from_proxy_packet(const uint8_t *packet, size_t size, int accept_python_magic, char **errorMessage, uint64_t apiVersion);

/* ---- filters whose reference implementation is Python-side ---- */
/* ColorizeFilter._mapcolor (reference python/cwipc/filters/colorize.py:100-119): lut = 256x3 doubles, valid = 256 flags. */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_colorize(cwipc_pointcloud *pc, double weight, const double *lut, const uint8_t *valid);
/* SimulatecamsFilter, hard assignment (reference python/cwipc/filters/simulatecams.py:44-70): tile = 1 << c for the camera direction
 * (camera_dirs: cos, sin of 2 pi c / ncamera, as doubles) with the largest dot product with the point's position minus the
 * centroid, y ignored.  The centroid (numpy.mean of the float32 coordinates) is computed by the caller, as the reference does. */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_simulatecams(cwipc_pointcloud *pc, int ncamera, float centroid_x, float centroid_z, const double *camera_dirs);
/* ---- the seeded random filters ----
 * Their draws are stateless, keyed by a 64-bit seed, a tag per filter and a counter (csrc/counter_rng.hpp; tests/scene_model.py is
 * the numpy statement):
 *   GOLDEN          = 0x9E3779B97F4A7C15
 *   mix(z)          = the splitmix64 output function (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31)
 *   base(seed, tag) = mix((seed + tag) mod 2^64)         tag = 0x6e6f697365 ("noise") or 0x63616d73 ("cams")
 *   draw(b, k)      = mix((b + (k + 1) * GOLDEN) mod 2^64)       k = 0, 1, 2, ...
 *   u01(x)          = (double)(x >> 11) * 2^-53           in [0, 1)
 * Reproducible from the seed; not numpy's Mersenne stream, which the reference draws from.
 *
 * SimulatecamsFilter, soft assignment (reference python/cwipc/filters/simulatecams.py:60-69): the dot products are those of
 * cwipc_hip_simulatecams; `first` and `second` are the top two of the descending order by (value, camera index), of equal dot
 * products the higher index first.  With u = u01(draw(base(seed, cams), i)) for point i: w0 = d_first ** skew, w1 = d_second ** skew
 * (the dot products themselves when skew == 1.0), chance = -w0 + (w1 + w0) * u in f64, every step rounded; tile = 1 << first if
 * chance < 0, else 1 << second (so a NaN chance takes `second`, as in the reference).  The coordinate planes are shared with the
 * input.  NULL (logged) for ncamera < 2 -- the reference raises IndexError -- or > 32. */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_simulatecams_soft(cwipc_pointcloud *pc, int ncamera, float centroid_x, float centroid_z,
                                                                 const double *camera_dirs, double skew, uint64_t seed);
/* NoiseFilter (reference python/cwipc/filters/noise.py:31-50): every point moved along a random vector of length up to `distance`.  For
 * point i, with b = base(seed, noise) and u_j = u01(draw(b, 4 i + j)), in f64, every operation rounded once, in this order:
 *   v_c = -1.0 + 2.0 * u_c  (c = 0, 1, 2);  s = (v_0*v_0 + v_1*v_1) + v_2*v_2;  scale = sqrt(s) / u_3;  n_c = (v_c / scale) * distance;
 *   out_c = (float)((double)p_c + n_c)
 * -- numpy's uniform(-1, 1), linalg.norm(axis=1), rnd_vec / (norm / unif) * distance and `float32 += float64`.  IEEE at the edges:
 * u_3 == 0 gives an infinite scale and no noise, s == 0 gives NaN, non-finite coordinates propagate.  Colours and tiles are the
 * input's very words (shared, not copied); timestamp and cellsize are kept; an empty cloud gives an empty cloud. */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_noise(cwipc_pointcloud *pc, double distance, uint64_t seed);
/* cwipc_join_multi (reference python/cwipc/util.py:1330-1332): same result as the left fold of cwipc_join, one pass. */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_join_multi(cwipc_pointcloud **pcs, int npc);
/* p' = R p + t for a row-major 4x4 matrix (last row ignored), in f64, stored as float: what the reference's
 * cwipc_transform does through numpy (python/cwipc/registration/util.py:295-309). */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_transform(cwipc_pointcloud *pc, const double *matrix4x4);
/* Every point projected onto the plane y = 0 (MultiCameraToFloor's floor cloud): x, z, colours and tiles kept, y = +0.0, timestamp 0,
 * cellsize 0.  A copy of two planes and a memset on the device.  NULL (logged) on failure. */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_flatten_y(cwipc_pointcloud *pc);
/* p' = (p + (x, y, z)) * scale in f64, cellsize * scale: the reference's TransformFilter loop (python/cwipc/filters/transform.py:38-52). */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_offset_scale(cwipc_pointcloud *pc, double x, double y, double z, double scale);
/* used256[t] = 1 for every tile value t that occurs (python/cwipc/registration/util.py:285-293, get_tiles_used); returns how many, -1 on error. */
_CWIPC_UTIL_EXPORT int cwipc_hip_tiles_used(cwipc_pointcloud *pc, uint8_t *used256);
/* cwipc_tilefilter_masked (reference python/cwipc/registration/util.py:98-112): keep points with (tile & mask) != 0. */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_tilefilter_masked(cwipc_pointcloud *pc, int mask);
/* cwipc_direction_filter (reference python/cwipc/registration/util.py:114-143): the points whose normal faces (dx, dy, dz).  Normal =
 * unit eigenvector of the smallest eigenvalue of the covariance of the max_nn nearest points within radius (the point itself among
 * them; (0, 0, 1) for fewer than 3 such points or a zero covariance), turned to point away from the cloud's centroid; a point is
 * kept iff normal . d / |d| >= threshold (d unnormalised when it is 0).  Input order, rgb, tile, timestamp and cellsize are kept.
 * The reference's radius and max_nn are 0.02 and 30.  NULL on error (logged), also for radius <= 0 or not finite, max_nn < 1 or > 128. */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_direction_filter(cwipc_pointcloud *pc, double dx, double dy, double dz, double threshold, float radius, int max_nn);

/* ---- Euclidean clusters: the connected components of "closer than radius" (what PCL users know as EuclideanClusterExtraction; no
 * reference counterpart).  The clean-up that stands beside cwipc_remove_outliers in a chain: a density test passes a dense clump of
 * flying pixels, a size test on its component does not.  tests/cluster_model.py is the numpy and scipy model of this text.
 *
 * RULE K.
 *  Links.     Points i != j are linked iff both have three finite coordinates and d2 < r2, strictly:  dx = (double)x_i - (double)x_j,
 *             dy, dz alike;  d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded on its own;  r2 = radius * radius in float64 --
 *             the arithmetic and the strictness of cwipc_hip_correspondences.  Identical coordinates are linked whenever r2 > 0 (d2 = 0 < r2);
 *             a radius below about 1.5e-162 is accepted, squares to r2 = 0 and links nothing, not even identical coordinates.
 *             A radius above about 1.3e154 squares to r2 = inf and links every pair of finite points.
 *             With CWIPC_HIP_CLUSTER_SAME_TILE a link also needs equal tile bytes.
 *  Clusters.  The connected components of that graph.  A component's ROOT is its smallest original index.  Clusters are numbered
 *             0 .. C - 1 in ascending order of root, that is, in order of first appearance in the input.  label[i] is the number of
 *             i's cluster, sizes[c] its point count.  A point with a non-finite coordinate has label 0xFFFFFFFF: it belongs to no
 *             cluster and links to nothing.  Nothing in the result depends on grid layout, launch shape or scheduling.
 *  Ranking.   Clusters are ranked by (size descending, number ascending).
 *  Filter.    Point i is kept iff its cluster's size is at least min_points AND its cluster's rank is below max_clusters
 *             (max_clusters == 0: no limit).  Kept points keep input order, colours, tiles; timestamp and cellsize are the input's.
 *             Unlabelled points are dropped.  An empty cloud gives an empty cloud.
 *  Refusals.  -1 / NULL, logged as an ERROR, before anything is launched: a NULL cloud, a radius that is NaN, infinite or <= 0, flag
 *             bits other than the one below, a cap below the cloud's count (with labels or sizes given).
 * The cloud is neither consumed nor changed.  Cost grows with the number of points within radius of a point: a radius beyond the
 * whole cloud is n * n / 2 distance tests. */
#define CWIPC_HIP_CLUSTER_SAME_TILE 1
/* labels, sizes: host arrays of cap >= count(pc) entries, either may be NULL; the first *nclusters entries of sizes are written,
 * *nclusters <= count(pc).  One wait.  0 ok. */
_CWIPC_UTIL_EXPORT int cwipc_hip_clusters(cwipc_pointcloud *pc, double radius, int flags, uint32_t *labels, uint32_t *sizes, size_t cap, uint32_t *nclusters);
/* The filter.  The result is device-resident like every other filter's; the call waits once, for the count that sizes its result
 * (clouds of 2^20 points and more: and where the point grid's sparse layout waits, as every search on it does). */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_cluster_filter(cwipc_pointcloud *pc, double radius, int flags, uint64_t min_points, uint32_t max_clusters);
/* What the link kernel did, for measurements (the labels are computed and thrown away; the counting kernel is a variant of its own, a
 * little slower): stats[0] links seen, each unordered pair once; [1] unions issued (links not skipped because the other end already
 * hung under the lane's root); [2] parent words loaded by all finds; [3] the most loaded by one union.  These depend on scheduling.  0 ok. */
_CWIPC_UTIL_EXPORT int cwipc_hip_cluster_link_stats(cwipc_pointcloud *pc, double radius, int flags, uint64_t stats[4]);
/* An entry for tests: RULE K's Ranking and Filter on sizes that the caller gives -- a cluster of 2^24 points needs a cloud of 16 M
 * points, a size word of 2^24 does not.  The filter's own ranking and keep kernels run as if cluster c consisted of the one point c:
 * keep[c] = 1 iff sizes[c] >= min_points AND c's rank is below max_clusters (0: no limit), else 0.  A size of 0, which no cloud
 * produces, ranks last like any other value.  One wait.  0 ok; nclusters == 0 is ok and writes nothing; -1 (logged) for a NULL
 * pointer or nclusters >= 2^32 - 1. */
_CWIPC_UTIL_EXPORT int cwipc_hip_cluster_rank_keep(const uint32_t *sizes, size_t nclusters, uint64_t min_points, uint32_t max_clusters, uint8_t *keep);

/* ---- fixed-radius neighbourhoods: neighbour counts, radius outlier removal (what PCL users know as RadiusOutlierRemoval) and
 * first-order moving-least-squares smoothing (PCL's MovingLeastSquares without a polynomial: each point moved onto the plane fitted
 * to its neighbourhood); no reference counterpart.  The radius is a distance in the cloud's units, so the outlier test can be set once
 * for a rig -- cwipc_remove_outliers removes a share of any cloud, however clean -- and smoothing removes no point at all.
 * tests/neigh_model.py is the numpy and scipy model of this text; csrc/smooth_terms.hpp holds the per-point arithmetic of Smoothing.
 *
 * RULE N.
 *  Arithmetic.     All of it float64, every operation rounded on its own; the order written here is the contract.
 *  Neighbourhood.  r2 = radius * radius.  For points i, j with three finite coordinates each:  d_a = (double)p_j[a] - (double)p_i[a];
 *                  d2 = (d_x*d_x + d_y*d_y) + d_z*d_z;  N(i) = { j finite : d2 < r2 }, strictly, as in RULE K; i itself is in N(i)
 *                  whenever r2 > 0.  With CWIPC_HIP_NEIGH_SAME_TILE only j with i's tile byte belong.  A point with a non-finite
 *                  coordinate is nobody's neighbour and has N = {}.
 *  Counts.         count[i] = |N(i)| - 1 for a finite point, 0 for a non-finite one.  The radius at its extremes as in RULE K: r2 == 0
 *                  gives all zeros, r2 == inf every finite point of the same tile set.
 *  Outlier filter. Point i is kept iff it is finite and count[i] >= min_neighbours.  Kept points keep input order, colours, tiles;
 *                  timestamp and cellsize are the input's.
 *  Smoothing.      s = 65536.0 / radius.  Per neighbour j of i, i itself included:  o_a = (int64) rint(d_a * s), so |o_a| <= 65536;
 *                  t = 1.0 - d2 / r2;  w = (int64) rint(4096.0 * (t * t)) -- a compact biweight kernel, no exp.  Exact integer sums
 *                  in 64-bit words with wrapping arithmetic:  W = sum w;  S1_a = sum w * o_a;  S2_ab = sum w * o_a * o_b (six);
 *                  cnt = |N(i)|.  A term is at most 2^44: the sums are exact for cnt <= 2^18.
 *                  Point i is MOVED iff it is finite AND cnt - 1 >= max(2, min_neighbours) AND cnt <= 262144; otherwise its
 *                  coordinates are copied bit for bit.  For a moved point:  M_ab = (double)W * (double)S2_ab - (double)S1_a * (double)S1_b
 *                  (int64 -> double rounds to nearest even);  n = smallest_eigvec(M) (csrc/smallest_eigvec.hpp);  c_a = (double)S1_a /
 *                  (double)W;  h = (n_x*c_x + n_y*c_y) + n_z*c_z;  p'_a = (float)((double)p_a + (n_a * h) / s).  The sign of n cancels.
 *                  Colours, tiles, order, count, timestamp and cellsize are the input's.
 *  Nothing in a result depends on grid layout, launch shape, the order of points inside a cell, or scheduling.
 *  Refusals.       -1 / NULL, logged as an ERROR, before anything is launched: a NULL cloud, flag bits other than the one below, a cap
 *                  below the cloud's count; for counts and the outlier filter a radius that is NaN, infinite or <= 0 (RULE K's); for
 *                  smoothing a radius that is not finite or lies outside [1e-30, 1e30].
 * The cloud is neither consumed nor changed; an empty cloud gives an empty cloud (0 for the counts).  Cost grows with the number of
 * points within radius of a point. */
#define CWIPC_HIP_NEIGH_SAME_TILE 1
/* counts: a host array of cap >= count(pc) entries.  One wait.  0 ok. */
_CWIPC_UTIL_EXPORT int cwipc_hip_radius_counts(cwipc_pointcloud *pc, double radius, int flags, uint32_t *counts, size_t cap);
/* The outlier filter.  The result is device-resident; the call waits once, for the count that sizes its result (and where the point
 * grid's sparse layout waits, as every search on it does). */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_radius_outlier_filter(cwipc_pointcloud *pc, double radius, int flags, uint64_t min_neighbours);
/* Smoothing.  The result is device-resident, shares the input's colour / tile words and is handed back with the kernel in flight: the
 * call does not wait (but where the point grid's sparse layout does). */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_smooth(cwipc_pointcloud *pc, double radius, int flags, uint32_t min_neighbours);
/* The host twin of cwipc_hip_smooth: the same header text (csrc/smooth_terms.hpp) by brute force over all pairs, O(n * n), no GPU.
 * out: n points, not overlapping pts.  0 ok; -1 (logged) for NULL pointers with n > 0 and for what cwipc_hip_smooth refuses. */
_CWIPC_UTIL_EXPORT int cwipc_hip_smooth_host(const struct cwipc_point *pts, size_t n, double radius, int flags, uint32_t min_neighbours, struct cwipc_point *out);

/* ---- floor and tile helpers of the registration pipeline (reference python/cwipc/registration/util.py:146-229) ----
 * A point is FLOOR iff (double)y < level; a NaN y is not floor.  The reference compares the float32 column with a Python scalar,
 * which numpy rounds to float32 first: the caller passes that value (the Python wrappers do).  NULL (or -1) on error (logged):
 * a NULL cloud, no usable GPU.  Results carry the input's timestamp and cellsize 0 -- the cellsize of a cloud fresh from
 * cwipc_from_points / cwipc_from_numpy_matrix, which is what the reference's helpers return (they do not copy the cellsize). */
#define CWIPC_HIP_FLOOR_KEEP_FLOOR 1     /* class A, first in the result: the floor points */
#define CWIPC_HIP_FLOOR_KEEP_REST 2      /* class B, behind them: the points that are not floor */
#define CWIPC_HIP_FLOOR_LIMIT_RADIUS 4   /* class A only holds floor points with (double)d < radius, d = sqrt((x*x + y*y) + z*z) in float32 */
/* Stable two-class partition: all class A points in input order, then all class B points in input order; *n_first (may be NULL)
 * receives the number of class A points.  cwipc_floor_filter = KEEP_REST (keep=False) or KEEP_FLOOR (keep=True);
 * cwipc_limit_floor_to_radius = all three flags. */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_floor_partition(cwipc_pointcloud *pc, double level, int flags, double radius, uint64_t *n_first);
/* cwipc_randomize_floor: floor points first, the others behind; floor point i (in that order) has key splitmix64(seed + (i + 1) *
 * 0x9E3779B97F4A7C15), perm is the stable ascending argsort of the keys, and position j keeps x, y, z, r, g, b and takes the tile of
 * floor point perm[j].  (The reference shuffles with numpy's Mersenne Twister; the contract here is a uniform permutation of the
 * floor's tiles that a seed reproduces.) */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_randomize_floor(cwipc_pointcloud *pc, double level, uint64_t seed);
/* What cwipc_compute_radius interpolates between, per class c (0 floor, 1 not floor) on d = sqrt((x*x + 0) + z*z) in float32:
 * count[c], stat[2 c] = sorted(d)[lo] and stat[2 c + 1] = sorted(d)[min(lo + 1, count[c] - 1)] with lo = floor((count[c] - 1) * 0.99),
 * the product in float32 as numpy.percentile computes it for float32 data; NaN for an empty class.  Exact (radix selection). 0 ok. */
_CWIPC_UTIL_EXPORT int cwipc_hip_floor_radius_stats(cwipc_pointcloud *pc, double level, uint64_t count[2], float stat[4]);
/* counts[t] = number of points with tile t, of all points or (nonfloor_only) of those that are not floor.  0 ok. */
_CWIPC_UTIL_EXPORT int cwipc_hip_tile_counts(cwipc_pointcloud *pc, int nonfloor_only, double level, uint64_t counts[256]);
/* minmax = min x, min y, min z, max x, max y, max z; NaN is skipped per coordinate (as Python's < and > do in the reference's
 * analyze filter); a coordinate without a value (an empty cloud) has min +inf and max -inf.  0 ok. */
_CWIPC_UTIL_EXPORT int cwipc_hip_bounds(cwipc_pointcloud *pc, float minmax[6]);

/* ---- plane segmentation: the dominant plane of a cloud by random-sample consensus (what PCL users know as SACSegmentation, open3d's
 * segment_plane), a refit over its inliers, the partition by a plane and the rotation that makes the plane y = 0; no reference
 * counterpart.  It is the entry of a cloud whose floor is NOT yet at y = 0 into the floor helpers above.  tests/plane_model.py is the
 * numpy model of this text; csrc/plane_seg_terms.hpp holds the per-hypothesis and per-point arithmetic.
 *
 * RULE S.
 *  Arithmetic.   All of it float64, every operation rounded on its own, in the order written here, no contraction.
 *  Parameters.   distance finite and within [1e-30, 1e30];  iterations = H in 1 .. 65536;  seed any uint64;  axis[3] and min_abs_cos
 *                in [0, 1] the optional constraint: min_abs_cos == 0 or a zero axis means unconstrained.  The caller passes a unit
 *                axis (the Python wrapper normalises it and turns an angle into the cosine: no trigonometry enters the rule).
 *                flags: CWIPC_HIP_PLANE_REFINE.
 *  Draws.        b = rng_base(seed, RNG_TAG_PLANE), RNG_TAG_PLANE = 0x706c616e65 ("plane"; csrc/counter_rng.hpp).  Hypothesis h takes
 *                x_k = rng_draw(b, 3 h + k), k = 0, 1, 2, and i_k = ((x_k >> 32) * n) >> 32 in 64-bit integers, n the cloud's count
 *                (< 2^32).  The constraint does not change which triples are drawn.
 *  Hypothesis.   p_k = point i_k as doubles;  u = p1 - p0;  v = p2 - p0;  c = (u_y v_z - u_z v_y, u_z v_x - u_x v_z, u_x v_y - u_y v_x);
 *                l2 = (c_x c_x + c_y c_y) + c_z c_z.  VALID iff the three indices differ AND all nine coordinates are finite AND l2 is
 *                finite and > 0 AND, with a constraint, |(n_x a_x + n_y a_y) + n_z a_z| >= min_abs_cos.  n = c / sqrt(l2), component
 *                by component;  d = -((n_x p0_x + n_y p0_y) + n_z p0_z).  The table row of an invalid hypothesis is four +0.0.
 *  Score.        e(p) = ((n_x x + n_y y) + n_z z) + d;  p is an INLIER iff fabs(e) <= distance (a non-finite point never is).
 *                count[h] = the number of inliers; 0 for an invalid hypothesis, which is not scored.
 *  Best.         Among the valid hypotheses the largest count, then the smallest h.  found = 0 when none is valid (n < 3 included):
 *                not an error.
 *  Refit.        (REFINE, over the best hypothesis' inliers.)  Anchor a = p0 of the best triple;  s = 16.0 / distance;
 *                o_a = rint((p_a - a_a) * s);  an inlier takes part iff all |o_a| <= 262144.  cnt, S1[3] = sum o_a, S2[6] = sum o_a o_b
 *                (xx xy xz yy yz zz) are exact 64-bit integers for cnt <= 2^26.  On the host M_ab = cnt * S2_ab - S1_a * S1_b exactly in
 *                128-bit integers, converted to double once (to nearest even);  n' = smallest_eigvec(M) (csrc/smallest_eigvec.hpp),
 *                turned so that (n'_x n_x + n'_y n_y) + n'_z n_z >= 0;  c_a = a_a + ((double)S1_a / (double)cnt) / s;
 *                d' = -((n'_x c_x + n'_y c_y) + n'_z c_z).  The score runs once more for (n', d') alone: the recount.  The refined
 *                plane is RETURNED iff 3 <= cnt <= 2^26 AND n' is finite AND the constraint holds for n' AND recount >= count;
 *                otherwise the hypothesis is.  `refined` says which.
 *  Orientation.  The returned plane (n, d) is negated (exactly) iff (n_x a_x + n_y a_y) + n_z a_z < 0, a the caller's axis, or
 *                (0, 1, 0) when unconstrained.  The hypothesis in the result is the table's row, not turned.
 *  Partition.    Class A: the inliers of a GIVEN plane and distance; with CWIPC_HIP_PLANE_BELOW_IS_INLIER the points with
 *                e <= distance (the floor and everything under it).  Class B: the other points, non-finite ones included.  A stable
 *                two-class partition with KEEP_INLIERS / KEEP_REST and *n_first as cwipc_hip_floor_partition has it; colours, tiles,
 *                timestamp and cellsize are the input's.
 *  Levelling.    A plane with n_y < 0 is negated first; (n, d) is divided by |n|.  R is the minimal rotation taking n to (0, 1, 0)
 *                (Rodrigues about n x Y): rows (1 - f n_x n_x, -n_x, -f n_x n_z), (n_x, n_y, n_z), (-f n_x n_z, -n_z, 1 - f n_z n_z) with
 *                f = 1 / (1 + n_y);  t = (0, d, 0).  Worked out in long double and rounded once, as plane_motion (csrc/plane_fit.hpp)
 *                does: every entry of R^T R - I stays within PLANE_FIT_ORTHO_BOUND.
 *  Refusals.     -1 / NULL, logged as an ERROR, before anything is launched: a NULL cloud or pointer, parameters outside the ranges
 *                above, unknown flag bits, for partition and levelling a non-finite plane, a zero normal or a distance that find refuses.
 *  Nothing depends on launch shape or scheduling: all device-side sums are integers.
 * The cloud is neither consumed nor changed.  Cost: count(pc) * iterations plane tests. */
#define CWIPC_HIP_PLANE_REFINE 1
#define CWIPC_HIP_PLANE_KEEP_INLIERS 1     /* class A, first in the result */
#define CWIPC_HIP_PLANE_KEEP_REST 2        /* class B, behind them */
#define CWIPC_HIP_PLANE_BELOW_IS_INLIER 4  /* class A is e <= distance instead of |e| <= distance */
#define CWIPC_HIP_PLANE_MAX_ITERATIONS 65536
typedef struct cwipc_hip_plane_params {
    double distance;
    uint64_t seed;
    double axis[3];
    double min_abs_cos;
    uint32_t iterations;
    int32_t flags;
} cwipc_hip_plane_params;
typedef struct cwipc_hip_plane_result {
    double plane[4];        /* the returned plane n_x, n_y, n_z, d (oriented); zeros when found == 0 */
    double hypothesis[4];   /* the best hypothesis' table row */
    int64_t sums[10];       /* the refit's cnt, S1[3], S2[6]; zeros without REFINE */
    double M[6];            /* the refit's matrix xx xy xz yy yz zz; zeros unless 3 <= cnt <= 2^26 */
    uint32_t best;          /* h of the best hypothesis */
    uint32_t triple[3];     /* its point indices */
    uint32_t count;         /* its inliers */
    uint32_t recount;       /* inliers of the refit plane (0 when it was not scored) */
    uint32_t valid;         /* number of valid hypotheses */
    int32_t found;
    int32_t refined;        /* 1: plane is the refit's, 0: the hypothesis' */
    int32_t reserved;
} cwipc_hip_plane_result;
/* The dominant plane.  Without REFINE one wait; with it one for best and sums (chained on the device), a host solve, one for the
 * recount.  0 ok (found == 0 included). */
_CWIPC_UTIL_EXPORT int cwipc_hip_plane_find(cwipc_pointcloud *pc, const cwipc_hip_plane_params *params, cwipc_hip_plane_result *result);
/* The whole table, for tests and diagnostics: planes (4 H doubles), counts (H), triples (3 H), valid (H bytes); each may be NULL. */
_CWIPC_UTIL_EXPORT int cwipc_hip_plane_scores(cwipc_pointcloud *pc, const cwipc_hip_plane_params *params, double *planes, uint32_t *counts, uint32_t *triples,
                                              uint8_t *valid);
/* Partition by a given plane.  The result is device-resident; two waits as the floor partition's. */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_plane_partition(cwipc_pointcloud *pc, const double plane[4], double distance, int flags, uint64_t *n_first);
/* Levelling: m16 = the row-major 4x4 [R t; 0 1] that cwipc_hip_transform takes.  Host only, no GPU.  0 ok. */
_CWIPC_UTIL_EXPORT int cwipc_hip_plane_level_matrix(const double plane[4], double m16[16]);
/* The host twin of cwipc_hip_plane_find and cwipc_hip_plane_scores: the same header text by brute force, O(n * H), no GPU.  planes,
 * counts and valid as above, each may be NULL.  0 ok; -1 (logged) for what cwipc_hip_plane_find refuses and n >= 2^32. */
_CWIPC_UTIL_EXPORT int cwipc_hip_plane_find_host(const struct cwipc_point *pts, size_t n, const cwipc_hip_plane_params *params, cwipc_hip_plane_result *result,
                                                 double *planes, uint32_t *counts, uint8_t *valid);

/* ---- the registration analyzer's arithmetic (reference python/cwipc/registration/analyze.py) ---- */
/* Per point of `source` the SQUARED distance, in f64, to its (nth + 1)-th nearest point of `reference` among those closer than
 * max_distance (strictly; INFINITY: no bound), +inf when there are fewer: d2 = (dx*dx + dy*dy) + dz*dz with dx = (double)qx - (double)px,
 * every operation rounded on its own -- sqrt(d2) is what scipy.spatial.KDTree.query(points, k=[nth + 1], distance_upper_bound=max_distance)
 * returns, bit for bit.  dist2: host array of cap >= count(source) doubles, in the source's order.  The clouds may be the same one
 * (the point itself is then the nearest, at 0) and are neither consumed nor changed.  An empty source writes nothing, an empty
 * reference gives +inf everywhere.  0 ok; -1 (logged) for a NULL cloud, nth < 0 or > 31, max_distance NaN or <= 0, cap too small. */
_CWIPC_UTIL_EXPORT int cwipc_hip_nn_distance2(cwipc_pointcloud *source, cwipc_pointcloud *reference, int nth, double max_distance, double *dist2, size_t cap);
/* The same search for up to 64 JOBS over one pair of clouds in one call (registration/multicamera.py: every camera of a frame against
 * the others): a job names the points that take part by a tile mask and an open y interval per side, instead of by filtered clouds.
 * dist2: host array of njobs rows of cap >= count(source) doubles; dist2[j * cap + i] is NaN where source point i takes no part in job
 * j, otherwise the squared distance (the arithmetic above) to its (nth + 1)-th nearest PARTICIPATING reference point strictly under
 * max_distance, +inf where there is none -- the bits cwipc_hip_nn_distance2 gives for the two filtered clouds.  The clouds may be the
 * same one (the point itself is then a candidate if it takes part as a reference point); they are neither consumed nor changed.
 * The y limits in the doubles the floor predicates use: ignore_floor (y > float32(0.1)) is {(double)float32(0.1), +inf} on both sides,
 * cwipc_floor_filter(keep=True) (y < float32(level)) is {-inf, (double)float32(level)}.  0 ok; -1 (logged) for a NULL cloud, njobs
 * outside 1..64, a job with nth outside 0..31, max_distance NaN or <= 0 or a NaN y limit, cap too small. */
typedef struct cwipc_hip_nn_job {
    uint8_t  source_mask;      /* a source point takes part iff (tile & source_mask) != 0; 0: every source point */
    uint8_t  reference_mask;   /* the same for reference points */
    int32_t  nth;              /* 0..31, as cwipc_hip_nn_distance2 */
    double   max_distance;     /* > 0, INFINITY: no bound */
    double   source_y[2];      /* a source point takes part iff source_y[0] < (double)y < source_y[1]; -inf / +inf: no limit */
    double   reference_y[2];   /* the same for reference points */
} cwipc_hip_nn_job;
_CWIPC_UTIL_EXPORT int cwipc_hip_nn_distance2_jobs(cwipc_pointcloud *source, cwipc_pointcloud *reference, const cwipc_hip_nn_job *jobs, int njobs,
                                                   double *dist2, size_t cap);
/* 1-D Gaussian kernel density estimate: density[j] = sum_i exp(-0.5 ((at[j] - samples[i]) / h)^2) / (n h sqrt(2 pi)) in f64, summed in
 * an order fixed by n (what scipy.stats.gaussian_kde(samples).evaluate(at) computes for h = std(samples, ddof=1) * factor).  Host
 * arrays: n samples, m evaluation points, m densities.  0 ok; -1 (logged) for n == 0, h not finite or <= 0, a NULL array. */
_CWIPC_UTIL_EXPORT int cwipc_hip_gaussian_kde(const double *samples, size_t n, double h, const double *at, size_t m, double *density);

/* ---- point-to-point ICP (reference python/cwipc/registration/fine.py, and analyze.py's OverlapAnalyzer: open3d's registration_icp
 * and evaluate_registration) ----
 * Matrices are 16 doubles, a row-major 4x4 whose last row is taken for (0, 0, 0, 1).  A source point (x, y, z) is moved in f64:
 * px = ((T00*x + T01*y) + T02*z) + T03 (py, pz alike), every operation rounded on its own.  Its correspondence is the reference point
 * with the smallest d2 = (dx*dx + dy*dy) + dz*dz, dx = px - (double)qx, among those with d2 < max_distance^2 (strictly; INFINITY: no
 * bound); among equal d2 the smallest index.  A source point with a non-finite coordinate (before or after T) has none; a reference
 * point with a non-finite coordinate is never one.  The clouds are neither consumed nor changed.  All three return 0, or -1 (logged)
 * for a NULL cloud, max_distance NaN or <= 0, a matrix that is not finite. */
/* idx[i] = index of source point i's correspondence in the reference (0xFFFFFFFF: none), dist2[i] = its d2 (+inf: none); host arrays
 * of cap >= count(source) entries, either may be NULL.  T NULL: the identity.  An empty reference gives none everywhere, an empty
 * source writes nothing.  -1 also for a cap that is too small. */
_CWIPC_UTIL_EXPORT int cwipc_hip_correspondences(cwipc_pointcloud *source, cwipc_pointcloud *reference, const double *T, double max_distance,
                                                 uint32_t *idx, double *dist2, size_t cap);
/* One search and the sums of a rigid fit over the source points that have a correspondence, nothing per point leaves the device:
 * with a = p - cp (p the moved source point) and b = q - cq (q its correspondence), *n = their number and
 * sums = sum a (3) | sum b (3) | sum a b^T (9, row-major a_i b_j) | sum d2, in f64, summed in an order fixed by count(source): the
 * same clouds give the same bytes.  T, cp, cq NULL: the identity, (0, 0, 0).  n and sums may be NULL.  With T the identity, n / count(source)
 * and sqrt(sums[15] / n) are the fitness and inlier_rmse of open3d's evaluate_registration. */
_CWIPC_UTIL_EXPORT int cwipc_hip_icp_sums(cwipc_pointcloud *source, cwipc_pointcloud *reference, const double *T, double max_distance,
                                          const double *cp, const double *cq, uint64_t *n, double *sums);
/* open3d's registration_icp with TransformationEstimationPointToPoint: evaluate at T = init (NULL: the identity); without a
 * correspondence return init, fitness 0, rmse 0; else up to max_iteration times: update = the rigid fit (umeyama without scaling) of
 * the correspondences, T = update * T, evaluate again, stop when |fitness change| < relative_fitness and |rmse change| < relative_rmse.
 * fitness = n / count(source), inlier_rmse = sqrt(sum d2 / n).  T is applied to the original float32 source points in every
 * iteration (open3d moves an f64 copy of the cloud step by step).  The outputs may be NULL.  -1 also for max_iteration < 0. */
_CWIPC_UTIL_EXPORT int cwipc_hip_icp_point2point(cwipc_pointcloud *source, cwipc_pointcloud *reference, double max_distance, const double *init,
                                                 double relative_fitness, double relative_rmse, int max_iteration, double *T_out, double *fitness,
                                                 double *inlier_rmse, int *iterations);

/* ---- point-to-plane ICP (reference python/cwipc/registration/fine.py: open3d's registration_icp with
 * TransformationEstimationPointToPlane) ----
 * open3d is not on this stack: the contract is a restatement of open3d's estimate, pinned by a numpy model.  Correspondences are
 * exactly those of cwipc_hip_correspondences.  For a matched pair, every operation rounded on its own: p the moved source point,
 * q the matched reference point, m that reference point's normal (q, m: (double) of float32), e = p - q,
 * r = (e0*m0 + e1*m1) + e2*m2, c = p x m (c0 = p1*m2 - p2*m1, c1 = p2*m0 - p0*m2, c2 = p0*m1 - p1*m0), J = (c0, c1, c2, m0, m1, m2);
 * no pivots.  Negating a normal leaves every term's bits unchanged: the orientation of the normals does not matter.
 * normals: the REFERENCE cloud's, three planes of count(reference) floats, x then y then z (the layout cwipc_hip_estimate_normals
 * writes, with cap = count(reference)), in host memory; NULL: estimated on the device as cwipc_hip_estimate_normals(radius, max_nn)
 * does, once per call (open3d's KDTreeSearchParamHybrid; the reference uses 0.02 and 30).  The source's normals are never read.
 * Errors as for the point-to-point entries; -1 also for a normal that is not finite and, with normals NULL, for radius <= 0 or not
 * finite, max_nn < 1 or > 128. */
/* One search and the sums of a plane fit: *n = the number of matched pairs,
 * sums = sum J_i J_j for i <= j (21, the upper triangle row-major) | sum J_i r (6) | sum r^2 | sum d2, 29 doubles, summed in an order
 * fixed by count(source): the same clouds give the same bytes.  T NULL: the identity.  n and sums may be NULL. */
_CWIPC_UTIL_EXPORT int cwipc_hip_icp_plane_sums(cwipc_pointcloud *source, cwipc_pointcloud *reference, const double *T, double max_distance,
                                                const float *normals, float radius, int max_nn, uint64_t *n, double *sums);
/* cwipc_hip_icp_point2point's loop with the point-to-plane update: A x = -b with A = sum J J^T, b = sum J r, by LDL^T with diagonal
 * pivoting in f64; the update is the identity when |det A| < 1e-6, a pivot is <= 0 or anything is not finite (open3d's check_det
 * rule), else R = Rz(x2) Ry(x1) Rx(x0), t = (x3, x4, x5).  fitness = n / count(source), inlier_rmse = sqrt(sum d2 / n): from the
 * point distances, not from r.  The same stop rule; T is applied to the original float32 source points in every iteration. */
_CWIPC_UTIL_EXPORT int cwipc_hip_icp_point2plane(cwipc_pointcloud *source, cwipc_pointcloud *reference, double max_distance, const double *init,
                                                 const float *normals, float radius, int max_nn, double relative_fitness, double relative_rmse,
                                                 int max_iteration, double *T_out, double *fitness, double *inlier_rmse, int *iterations);

/* ---- generalized ICP (reference python/cwipc/registration/fine.py, its default aligner: open3d's registration_generalized_icp with
 * TransformationEstimationForGeneralizedICP, epsilon 1e-3, L2 loss) ----
 * open3d is not on this stack: the contract is a restatement of the published algorithm, pinned by a numpy model.  Every operation is
 * rounded on its own, in f64.
 * NORMALS.  Both clouds have normals: the caller's (three planes of count floats, x then y then z, the layout
 * cwipc_hip_estimate_normals writes with cap = count) or, for NULL, estimated on the device as cwipc_hip_estimate_normals(radius,
 * max_nn) does, once per call and on the cloud as given (the source's on the original source cloud, not on the moved one).
 * ORIENTATION (the reference's _fix_normal_direction; open3d's OrientNormalsToAlignWithDirection).  cs, ct: the f64 means of the
 * source and the reference, o = (cs + ct) / 2; the source's direction is d = cs - o, the reference's d = ct - o.  Per normal m
 * ((double) of float32): all three components 0: m = d; else if (m0*d0 + m1*d1) + m2*d2 < 0: m = -m.  A comparison with NaN is
 * false, so a NaN direction never flips a normal.
 * COVARIANCE (open3d's GetRotationFromE1ToX and Rx diag(eps, 1, 1) Rx^T), per point, once per call, from the oriented normal:
 * c = m0; if c < -0.99, Rx = I (open3d's rule as published: the covariance is diag(eps, 1, 1) for every normal within about 8
 * degrees of -x); otherwise, with f = 1 / (1 + c),
 *     Rx = [[1 - f*(m1*m1 + m2*m2),  -m1,            -m2          ],
 *           [m1,                     1 - f*(m1*m1),  -(f*(m1*m2)) ],
 *           [m2,                     -(f*(m1*m2)),   1 - f*(m2*m2)]]
 * and C_ij = ((eps*Rx_i0)*Rx_j0 + Rx_i1*Rx_j1) + Rx_i2*Rx_j2 for i <= j: six values, in the order 00, 01, 02, 11, 12, 22.
 * PER MATCHED PAIR.  Correspondences are exactly those of cwipc_hip_correspondences.  p the moved source point, q the matched
 * reference point ((double) of float32), R the 3x3 block of T, Cs the source point's covariance, Ct the reference point's:
 *     B = R Cs:  B_ij = (R_i0*Cs_0j + R_i1*Cs_1j) + R_i2*Cs_2j;   S_ij = (B_i0*R_j0 + B_i1*R_j1) + B_i2*R_j2;   M_ij = Ct_ij + S_ij   (i <= j)
 *     k00 = M11*M22 - M12*M12,  k01 = M02*M12 - M01*M22,  k02 = M01*M12 - M02*M11,
 *     k11 = M00*M22 - M02*M02,  k12 = M01*M02 - M00*M12,  k22 = M00*M11 - M01*M01,
 *     det = (M00*k00 + M01*k01) + M02*k02,  N_ij = k_ij / det                                   (N = M^-1, symmetric)
 *     e = p - q,  g_i = (N_i0*e0 + N_i1*e1) + N_i2*e2
 *     A = [-skew(p) | I]: the rows (0, p2, -p1, 1, 0, 0), (-p2, 0, p0, 0, 1, 0), (p1, -p0, 0, 0, 0, 1)
 *     H = N A:  H_ij = (N_i0*A_0j + N_i1*A_1j) + N_i2*A_2j;   (A^T H)_ij = (A_0i*H_0j + A_1i*H_1j) + A_2i*H_2j   (i <= j)
 *     (A^T g)_i = (A_0i*g0 + A_1i*g1) + A_2i*g2,   e^T g = (e0*g0 + e1*g1) + e2*g2
 * open3d writes W = (M^-1)^(1/2), J = W A, r = W e; W is symmetric, so J^T J = A^T N A, J^T r = A^T g, r^T r = e^T g.
 * Errors as for the point-to-plane entries (either normals array NULL: radius and max_nn are checked); -1 also for an epsilon that
 * is not finite or <= 0. */
/* The covariances of one cloud, for parity tests: cov = count rows of the six values, host memory of cap >= count rows.  direction: 3
 * doubles, or NULL: no orientation step.  -1 also for a cap that is too small. */
_CWIPC_UTIL_EXPORT int cwipc_hip_gicp_covariances(cwipc_pointcloud *pc, const float *normals, float radius, int max_nn, const double *direction,
                                                  double epsilon, double *cov, size_t cap);
/* One search and the sums of a generalized fit, in the layout of the plane sums: *n = the number of matched pairs,
 * sums = sum (A^T N A)_ij for i <= j (21, the upper triangle row-major) | sum (A^T g)_i (6) | sum e^T g | sum d2, 29 doubles, summed
 * as the plane sums are: the same clouds give the same bytes.  Both directions come from the two clouds.  T NULL: the identity.  n
 * and sums may be NULL. */
_CWIPC_UTIL_EXPORT int cwipc_hip_icp_gicp_sums(cwipc_pointcloud *source, cwipc_pointcloud *reference, const double *T, double max_distance,
                                               const float *source_normals, const float *reference_normals, float radius, int max_nn, double epsilon,
                                               uint64_t *n, double *sums);
/* cwipc_hip_icp_point2plane's loop with these sums: the same 6x6 solve and check_det rule, R = Rz Ry Rx, fitness = n / count(source),
 * inlier_rmse = sqrt(sum d2 / n), the same stop rule.  T is applied to the original float32 source points, and its rotation to the
 * original source covariances, in every iteration (open3d moves an f64 copy of both step by step). */
_CWIPC_UTIL_EXPORT int cwipc_hip_icp_generalized(cwipc_pointcloud *source, cwipc_pointcloud *reference, double max_distance, const double *init,
                                                 const float *source_normals, const float *reference_normals, float radius, int max_nn, double epsilon,
                                                 double relative_fitness, double relative_rmse, int max_iteration, double *T_out, double *fitness,
                                                 double *inlier_rmse, int *iterations);

/* ---- cloud distortion: what a degraded cloud (a decoded packet, a downsampled or filtered cloud) lost against its original ----
 * No reference counterpart.  The measures are those of MPEG's pc_error -- point-to-point error (D1), point-to-plane error (D2),
 * colour error in BT.709 YUV, each in both directions -- the rule is this library's own, stated here once and pinned by a numpy
 * model (tests/quality_model.py); the arithmetic is csrc/quality_terms.hpp (host and device compile it).
 *
 * RULE Q.  Two clouds: `original`, called A, and `degraded`, called B.  Two passes; each is "every source point is matched to its
 * nearest reference point", with exactly the correspondences cwipc_hip_correspondences gives for T the identity:
 *   d2 = (dx*dx + dy*dy) + dz*dz in f64 from the float32 coordinates; only d2 < max_distance^2 (strictly; INFINITY: no bound); among
 *   equal d2 the smallest original index wins; a source point with a non-finite coordinate has no match; a non-finite reference
 *   point is never a match.
 *   BACKWARD (out[1]): source B, reference A.  The normal of a matched pair is A's normal at the matched index.  This pass runs
 *     first; its index array idxBA stays on the device.
 *   FORWARD (out[0]): source A, reference B.  Reference point j of B inherits the normal nA[idxBA[j]]; it has none when idxBA[j] is
 *     none.  The degraded cloud's own normals are never estimated: a decoded cloud is a lattice of cell centres, its normals mean
 *     nothing.
 * PER MATCHED PAIR, every operation rounded on its own in f64: p the source point, q the reference point, m the normal when there
 * is one, all (double) of float32:
 *     e = p - q,  r = (e0*m0 + e1*m1) + e2*m2
 *     dR, dG, dB = the source's colour byte minus the reference's, as doubles (integers in -255 .. 255)
 *     dY = (0.2126*dR + 0.7152*dG) + 0.0722*dB
 *     dU = (-0.1146*dR - 0.3854*dG) + 0.5*dB
 *     dV = (0.5*dR - 0.4542*dG) - 0.0458*dB                         (BT.709, as in pc_error; the offsets of 128 cancel)
 * and the pair's terms are  1 | 1.0 with a normal, 0.0 without | d2 | r*r (0.0 without a normal) | dR*dR, dG*dG, dB*dB | dY*dY,
 * dU*dU, dV*dV.  Negating a normal leaves every term's bits as they are.  Per pass the terms are summed over the matched pairs in
 * f64, in the order of the ICP sums (fixed by the source's count: the same clouds give the same bytes); the counts and the three RGB
 * sums are sums of integers below 2^53, exact in any order, and are handed out as integers.  Besides the sums: max_d2, the largest
 * d2 over the matched pairs, 0 when there are none.
 * From the sums (cwipc_util_amd.quality does this): mse_d1 = sum_d2 / n, mse_d2 = sum_r2 / n_plane, hausdorff = sqrt(max_d2),
 * mse of a colour channel = its sum / n; symmetric = the larger of the two directions; psnr = 10 log10(3 peak^2 / mse) for the
 * geometry and 10 log10(255^2 / mse) for a colour channel.
 * NOT pc_error's: a pair's normal is inherited through the nearest index (pc_error averages the normals of equally near points);
 * peak is the caller's (the Python layer takes the largest extent of the original's bounding box); there is no reflectance.
 *
 * normals: the ORIGINAL's, three planes of count(original) floats, x then y then z, in host memory; NULL: estimated on the device
 * as cwipc_hip_estimate_normals(radius, max_nn) does, once per call.  flags: CWIPC_HIP_DISTORTION_NO_PLANE or 0.  The clouds may be
 * the same one; they are neither consumed nor changed.  An empty cloud on either side gives n = 0 in both directions and returns 0
 * (n_source is the count of each pass's source all the same).  Nothing per point leaves the device.  0, or -1 (logged, nothing is
 * launched, out is zeroed) for a NULL cloud, max_distance NaN or <= 0, unknown flag bits, a NULL out and, without NO_PLANE, a normal
 * that is not finite or, with normals NULL, radius <= 0 or not finite, max_nn < 1 or > 128. */
#define CWIPC_HIP_DISTORTION_NO_PLANE 1   /* no normals are made or read: n_plane = 0, sum_r2 = 0 in both passes */
typedef struct cwipc_hip_distortion_sums {
    uint64_t n_source, n, n_plane;   /* the pass's source points; the matched pairs; those with a normal */
    double   sum_d2, max_d2, sum_r2;
    uint64_t sum_rgb2[3];
    double   sum_yuv2[3];
} cwipc_hip_distortion_sums;
_CWIPC_UTIL_EXPORT int cwipc_hip_distortion(cwipc_pointcloud *original, cwipc_pointcloud *degraded, double max_distance,
                                            const float *normals, float radius, int max_nn, int flags,
                                            cwipc_hip_distortion_sums out[2]);

/* ---- a cloud seen through a pinhole camera (reference python/cwipc/registration/multicoarse.py:333-360: MultiCameraCoarseAruco looks at
 * a camera's tile from the origin in an open3d window and grabs the window's colour and depth buffers) ----
 * Camera space looks along +z, image x runs right and image y down: the conventions of the reference's _deproject
 * (multicoarse.py:426-428, x = (u - cx) * z / fx, y = (v - cy) * z / fy).  extrinsic: world -> camera, a row-major 4x4 whose last row is
 * not read. */
typedef struct cwipc_hip_view {
    int32_t width, height;
    double fx, fy, cx, cy, near, far;
    double extrinsic[16];
} cwipc_hip_view;
/* Every point is drawn as a square of point_size x point_size pixels into a z-buffer.  Every operation is rounded on its own, in this
 * order, E = extrinsic, h = (point_size - 1) / 2:
 *  1. A point takes part iff (tilemask == 0 || (tile & tilemask) != 0) and x, y, z are finite.
 *  2. In f64 from the float32 coordinates: xc = ((E00*x + E01*y) + E02*z) + E03, yc and zc alike from rows 1 and 2.
 *  3. The point is dropped unless near < zc && zc < far.
 *  4. u = fx*(xc/zc) + cx, v = fy*(yc/zc) + cy.
 *  5. col = floor(u), row = floor(v); the point is dropped unless -(h+1) < floor(u) < width+h and -(h+1) < floor(v) < height+h, decided in
 *     f64 (a u or v that is not finite fails): no value is converted to an integer before it is known to fit.
 *  6. Its splat is every pixel (c, r) of the image with |c - col| <= h and |r - row| <= h.
 *  7. Its depth is (float)zc.  A pixel goes to the smallest depth, compared as float32; among equal depths to the smallest point index.
 *  8. Per pixel: depth = the winner's depth, rgb = its r, g, b, index = its position in the cloud (the unfiltered one, whatever the
 *     tilemask); a pixel no splat covers has depth 0.0f (what open3d's depth capture gives for the background), the background colour
 *     and index -1.
 * A pure function of its input: two calls give the same bytes.  rgb: height*width*3 bytes, depth: height*width floats, index:
 * height*width words or NULL, all row-major host arrays.  Returns the number of covered pixels; an empty cloud is all background and
 * returns 0.  -1 (cwipc_hip_last_error() has the text) for a NULL argument, width or height < 1, width*height > 2^24, a point_size that
 * is even or outside 1..15, near not > 0, far not > near, an intrinsic or extrinsic entry that is not finite (far may be INFINITY). */
_CWIPC_UTIL_EXPORT long cwipc_hip_render(cwipc_pointcloud *pc, const cwipc_hip_view *view, int point_size, int tilemask, const uint8_t background[3],
                                         uint8_t *rgb, float *depth, int32_t *index);

/* ---- square binary fiducials in an image (the reference finds them with cv2.aruco, python/cwipc/registration/multicoarse.py:492-527;
 * cv2 is no dependency of this project) ----
 * The markers have a 5 x 5 payload inside a one-cell black border, a 7 x 7 grid: the family of the reference's printable targets,
 * data/src/5x5_1000-N.svg.  dictionary[i] holds marker i's payload: bit 24 - (5*row + col) is the cell at row `row`, column `col`, a set
 * bit is a white cell; bits 25-31 are not looked at.  The package ships no bit patterns: the caller supplies them.
 * Every step is integer arithmetic; tests/marker_model.py restates it in numpy.  r = row, c = column, linear index = r*width + c: */
typedef struct cwipc_hip_marker_params {
    int32_t window_half;        /* default 40; 1..8192 */
    int32_t threshold_offset;   /* default 7;  0..255 */
    int32_t min_side;           /* default 14; 2..8192 */
    int32_t max_border_errors;  /* default 2;  0..24 */
    int32_t max_bit_errors;     /* default 0;  0..25 */
} cwipc_hip_marker_params;
/*  1. Grey.  Y = (77*R + 150*G + 29*B + 128) >> 8.
 *  2. Dark mask.  S = the sum of Y over the window [r-w, r+w] x [c-w, c+w], w = window_half, clipped to the image; n = the number of
 *     pixels in that clipped window.  A pixel is dark iff Y*n + threshold_offset*n < S.  S comes from a summed-area table in uint32
 *     (255 * 2^24 fits; width*height <= 2^24 as for the renderer).  The window is wide on purpose: every black pixel of a marker whose
 *     cells are narrower than w has white inside its window, so the whole border ring with every black cell 4-connected to it comes out
 *     as one blob.
 *  3. Components.  A component is a 4-connected set of dark pixels; its label is its smallest linear index.
 *  4. Candidate.  The component's bounding box touches no image edge and is at least min_side wide and high.
 *  5. Corners.  P0 = the label's pixel.  A = the component pixel farthest from P0 by squared distance, C = the one farthest from A.
 *     k(p) = (px-Ax)*(Cy-Ay) - (py-Ay)*(Cx-Ax) for every component pixel p; B = the pixel with the largest k, D = the one with the
 *     smallest.  Every tie goes to the smallest linear index.  Rejected unless k(B) > 0 > k(D), and unless A, B, C, D is strictly convex
 *     (the cross products of consecutive edges are all positive or all negative).  Of the two cycles A, B, C, D and A, D, C, B the one
 *     whose shoelace sum, sum(x_i*y_(i+1) - x_(i+1)*y_i), is positive is Q0..Q3, Q0 = A: clockwise on screen, because y runs down.
 *     Limit: this finds the corners of a quadrilateral whose diagonals are longer than its sides (a marker seen at any angle a camera
 *     can decode it from), not of a sliver whose longest chord is a side.
 *  6. Sampling.  The projective map that takes the square (0,0), (7,0), (7,7), (0,7) onto Q0..Q3, in Heckbert's closed form for
 *     square-to-quad: with dx1 = x1-x2, dx2 = x3-x2, sx = x0-x1+x2-x3 (dy1, dy2, sy alike), Dn = dx1*dy2 - dx2*dy1,
 *     G = sx*dy2 - dx2*sy, H = dx1*sy - sx*dy1, and U = 4*j + a, V = 4*i + b for the sample (j + a/4, i + b/4) of cell (i, j), a, b in
 *     {1, 2, 3}:
 *        numx = ((x1-x0)*Dn + G*x1)*U + ((x3-x0)*Dn + H*x3)*V + 28*x0*Dn   (numy alike),   den = G*U + H*V + 28*Dn;
 *     if den < 0 all three change sign; the sample's pixel is (floor((2*numx + den) / (2*den)), floor((2*numy + den) / (2*den))),
 *     i.e. floor(num/den + 1/2), by exact integer division.  A sample outside the image, or with den = 0, is not dark.  A cell is black
 *     iff at least 5 of its 9 sampled pixels are dark.
 *     Magnitudes, L = the larger side: |2*num + den| < 760 L^3 + 272 L^2, which int64 holds for L <= 2^17; the squared distances and
 *     k of step 5, < 2 L^2, are kept in 32 bits, which holds for L <= 2^14.  A side above 8192 is refused.
 *  7. Decode.  Rejected if more than max_border_errors of the 24 border cells are white.  The 25 inner cells form a code (white = 1).
 *     Rotation k means that the marker's canonical top-left corner is Q_k: the canonical cell (r, c) is the sampled inner cell (r, c),
 *     (c, 4-r), (4-r, 4-c), (4-c, r) for k = 0, 1, 2, 3.  The (id, k) of smallest Hamming distance to the dictionary is taken, ties to
 *     the smallest id, then the smallest k; accepted iff that distance is at most max_bit_errors.  The output corners are Q_k, Q_(k+1),
 *     Q_(k+2), Q_(k+3): cv2's order, top-left, top-right, bottom-right, bottom-left of the marker.  A mirrored marker does not decode.
 *  8. Output.  When an id is found more than once the candidate with the largest component area stays, ties to the smallest label.
 *     Sorted by id.  ids: cap words; corners: cap*4*2 floats, u then v, the integer pixel coordinates as floats.
 * Returns the number found; the first cap are written.  A pure function of the image.  -1 (cwipc_hip_last_error() has the text) for a
 * NULL argument (params may be NULL: the defaults; ids and corners may be NULL when cap is 0), width or height < 1 or > 8192,
 * width*height > 2^24, nmarkers < 1, a parameter outside the range given above. */
_CWIPC_UTIL_EXPORT long cwipc_hip_detect_markers(const uint8_t *rgb, int width, int height, const uint32_t *dictionary, int nmarkers,
                                                 const cwipc_hip_marker_params *params, int32_t *ids, float *corners, size_t cap);
/* cwipc_hip_render's kernels and the detector's on one stream; no image goes to the host.  corner_depth (cap*4 floats, may be NULL): the
 * depth image's value at each corner pixel.  ids, corners and corner_depth are, byte for byte, what cwipc_hip_render followed by
 * cwipc_hip_detect_markers on the host copy of its rgb image gives.  Errors: those of both calls. */
_CWIPC_UTIL_EXPORT long cwipc_hip_render_detect_markers(cwipc_pointcloud *pc, const cwipc_hip_view *view, int point_size, int tilemask,
                                                        const uint8_t background[3], const uint32_t *dictionary, int nmarkers,
                                                        const cwipc_hip_marker_params *params, int32_t *ids, float *corners, float *corner_depth,
                                                        size_t cap);

/* ---- the RGB-D source: a cloud from the cameras' own depth and colour images (the step a capturer plug-in of the reference does on
 * the host; its shared per-point filters: reference include/cwipc_util/internal/capturers.hpp:208-275) ---- */
typedef struct cwipc_hip_rgbd_camera {
    int32_t width, height;
    const uint16_t *depth;      /* Z16, row-major, 0: no depth */
    const uint8_t *colour;      /* ALIGNED to the depth image, the same size, rows tightly packed */
    int32_t bpp;                /* 3: R, G, B bytes; 4: B, G, R, A bytes */
    uint8_t tile;
    double fx, fy, cx, cy;
    double depth_scale;         /* metres per depth unit */
    double trafo[16];           /* camera -> world, row-major */
    const char *serial;         /* names the attached images; may be NULL when attach_flags is 0 */
} cwipc_hip_rgbd_camera;
typedef struct cwipc_hip_rgbd_filter {
    double threshold_near, threshold_far;   /* off when threshold_far <= threshold_near */
    double height_min, height_max;          /* off when height_min == height_max */
    float radius;                           /* off when radius <= 0 */
    int32_t greenscreen;                    /* off when 0 */
} cwipc_hip_rgbd_filter;
#define CWIPC_HIP_RGBD_ATTACH_RGB 1
#define CWIPC_HIP_RGBD_ATTACH_DEPTH 2
/* One device-resident cloud from ncam cameras' images.  All arithmetic is float64, every operation rounded on its own
 * (csrc/rgbd_terms.hpp is the one statement of it, tests/rgbd_model.py its numpy restatement).  Pixel (u, v) with depth d != 0:
 *    z  = (double)d * depth_scale;  xc = ((double)u - cx) * z / fx;  yc = ((double)v - cy) * z / fy      (left to right)
 *    X  = ((m00*xc + m01*yc) + m02*z) + m03, Y and Z alike, m = trafo;  the point is (float)X, (float)Y, (float)Z with the pixel's
 *    r, g, b and the camera's tile.
 * Filters, in this order (filter may be NULL: all off):
 *    depth range: dropped if z < threshold_near || z > threshold_far;
 *    height:      dropped if y < height_min || y > height_max, y the float32 world y;
 *    radius:      kept iff (float)((double)x*(double)x + (double)z*(double)z) < radius*radius (float32 product), x and z the float32
 *                 world coordinates: the reference's isPointInRadius;
 *    greenscreen: dropped iff the reference's integer hue (rgbToHsv) is in 60..130: what its isNotGreen comes to.
 * Output order: the cameras in argument order, within a camera the kept pixels in row-major order.  The images may be ordinary or
 * page-locked host memory (cwipc_hip_host_alloc / _register: then they are copied from where they lie); they go up with asynchronous
 * copies on the calling thread's stream and are free again when the call returns.  A frame in which nothing survives is a valid
 * empty cloud.  The cloud knows the tiles it can hold.  attach_flags (CWIPC_HIP_RGBD_ATTACH_*) copies the given images into the cloud's
 * metadata as "rgb.<serial>" ("width=W,height=H,bpp=3|4") and "depth.<serial>" ("width=W,height=H,bpp=2"), per camera in that order.
 * NULL (errorMessage, if given, and cwipc_hip_last_error() have the text) for a NULL pointer, ncam <= 0, a width or height < 1, more than
 * 2^31 - 1 pixels in all, bpp not 3 or 4, an intrinsic, depth_scale or matrix entry that is not finite, fx or fy zero. */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_from_rgbd(const cwipc_hip_rgbd_camera *cams, int ncam, const cwipc_hip_rgbd_filter *filter, uint64_t timestamp,
                                                         float cellsize, int attach_flags, char **errorMessage);
/* The two mappings a grabber answers for the registration tooling (auxiliary operations "map2d3d" and "mapcolordepth"), on the host,
 * with the arithmetic above.  map2d3d: the world point of colour pixel (u, v) at depth d (any u, v; d > 0); 1, or 0 for a NULL
 * argument, d <= 0, or a camera cwipc_hip_from_rgbd would refuse.  mapcolordepth: the depth pixel of colour pixel (u, v) -- the same
 * pixel, the images being aligned; 1 inside the image, 0 outside it or for a NULL argument. */
_CWIPC_UTIL_EXPORT int cwipc_hip_rgbd_map2d3d(const cwipc_hip_rgbd_camera *cam, int u, int v, int d, float out[3]);
_CWIPC_UTIL_EXPORT int cwipc_hip_rgbd_mapcolordepth(const cwipc_hip_rgbd_camera *cam, int u, int v, int out[2]);

/* ---- the RGB-D source's RAW entry: sensor pairs as a camera delivers them -- a depth image to be eroded, a colour image of another
 * size from a second sensor beside the first, both behind rational-model lenses.  The rules below are this project's own
 * definition (the camera plug-ins that hold the reference's versions are not in the reference tree); csrc/rgbd_lens.hpp is the one
 * statement of the arithmetic, tests/rgbd_lens_model.py its numpy restatement.  Float64, every operation rounded on its own. ---- */
typedef struct cwipc_hip_rgbd_sensor {
    int32_t width, height;              /* the depth image */
    double fx, fy, cx, cy;
    double coeffs[8];                   /* k1 k2 p1 p2 k3 k4 k5 k6, OpenCV's rational model; all zero: pinhole */
    double depth_scale;                 /* metres per depth unit */
    int32_t colour_width, colour_height;
    int32_t colour_bpp;                 /* 3: R, G, B bytes; 4: B, G, R, A bytes */
    double colour_fx, colour_fy, colour_cx, colour_cy;
    double colour_coeffs[8];
    double depth_to_colour[16];         /* row-major, depth-camera to colour-camera coordinates; taken as given, not judged */
    double trafo[16];                   /* camera -> world, row-major */
    uint8_t tile;
    const char *serial;                 /* names the attached images (copied by rig_create); may be NULL when nothing is ever attached */
} cwipc_hip_rgbd_sensor;
typedef struct cwipc_hip_rgbd_frame {
    const uint16_t *depth;              /* Z16, width x height, row-major, 0: no depth */
    const uint8_t *colour;              /* colour_width x colour_height x colour_bpp, rows tightly packed */
} cwipc_hip_rgbd_frame;
typedef struct cwipc_hip_rgbd_prep {
    int32_t depth_x_erosion, depth_y_erosion;   /* 0 .. 32 pixels, 0: off */
} cwipc_hip_rgbd_prep;
typedef struct cwipc_hip_rgbd_rig cwipc_hip_rgbd_rig;
/* What is constant per camera: the sensor table and every depth camera's ray table, computed here on the host and uploaded once (a
 * host copy stays for the mappings), and the device memory a frame needs.  Per grab only the images go up and the count comes back.
 * The ray table, entry (u, v):  xd = (u - cx) / fx;  yd = (v - cy) / fy;  all eight coefficients zero: (xd, yd); otherwise Newton's
 * method on distort(x, y) = (xd, yd) with the analytic Jacobian, from (xd, yd), at most 20 steps, accepted when |ex| < 1e-12 and
 * |ey| < 1e-12 and the Jacobian's determinant there is positive; anything else: (NaN, NaN), the pixel has no ray and gives no point.
 *    distort(x, y):  xx = x*x;  yy = y*y;  r2 = xx + yy
 *                    rad = (1 + r2*(k1 + r2*(k2 + r2*k3))) / (1 + r2*(k4 + r2*(k5 + r2*k6)))
 *                    a1 = (2*x)*y;  a2 = r2 + 2*xx;  a3 = r2 + 2*yy
 *                    x' = (x*rad + p1*a1) + p2*a2;   y' = (y*rad + p1*a3) + p2*a1
 * NULL (errorMessage, if given, and cwipc_hip_last_error() have the text) for a NULL pointer, ncam <= 0, a width or height < 1 (either
 * image), more than 2^31 - 1 depth pixels in all or colour pixels in one image, colour_bpp not 3 or 4, an intrinsic, coefficient,
 * depth_scale or matrix entry that is not finite, a focal length that is zero.  One grab at a time per rig (calls are serialised). */
_CWIPC_UTIL_EXPORT cwipc_hip_rgbd_rig *cwipc_hip_rgbd_rig_create(const cwipc_hip_rgbd_sensor *sensors, int ncam, char **errorMessage);
_CWIPC_UTIL_EXPORT void cwipc_hip_rgbd_rig_free(cwipc_hip_rgbd_rig *rig);
/* A rig that DECIMATES its depth images by `decimation` = k (1 .. 8) on the device, as the first step of every grab entry.
 * Such a rig is handed FULL-SIZE frames, width x height depth pixels as the sensor delivers them; everything after the decimation
 * lives on the decimated grid with DERIVED sensors: rules 0a - 0c and their per-pixel state, erosion, ray table, registration,
 * occlusion, compaction, the attached "depth.<serial>" / "rgb.<serial>" images and their "width=..,height=.." strings, rig_history,
 * rig_ray_table, rig_map2d3d and rig_mapcolordepth.  This project's own definition (the camera plug-ins that hold the vendors'
 * versions are not in the reference tree); csrc/rgbd_decimate.hpp is the one statement of it, tests/rgbd_decimate_model.py its numpy
 * restatement.
 * RULE D.  Arithmetic is float64, every operation rounded on its own;  q(x) = (uint16) floor(x + 0.5)  as in rule 0.
 *   The derived sensor:  W' = W div k;  H' = H div k.  Source columns from k*W' and rows from k*H' onward are never read.
 *     fx' = fx / k;  fy' = fy / k;  cx' = (cx - (k - 1) * 0.5) / k;  cy' alike: decimated pixel U sits at the centre of source pixels
 *     kU .. kU + k - 1.  The lens coefficients, depth_scale, every colour-side field, both matrices and the tile are unchanged.  The ray
 *     table is the rule above on the derived sensor, and the pinhole exception of rule 2 uses fx' and cx'.
 *   The value of decimated pixel (U, V), n the number of NON-ZERO values among the k * k source pixels (kU + i, kV + j), 0 <= i, j < k:
 *     n == 0:       0
 *     k = 2 or 3:   the LOWER MEDIAN: with the non-zero values sorted ascending, a[(n - 1) div 2]
 *     k = 4 .. 8:   q((double) sum / (double) n), sum the exact integer sum of the non-zero values
 *   The result lies in 1 .. 65535 whenever n > 0: no clamp is part of the rule.
 * decimation == 1 is cwipc_hip_rgbd_rig_create itself, byte for byte in everything observable.  NULL (the text in errorMessage and
 * cwipc_hip_last_error(), nothing allocated) for a decimation outside 1 .. 8, a sensor with width < k or height < k, and everything
 * cwipc_hip_rgbd_rig_create refuses (its limit of 2^31 - 1 depth pixels counts the full-size images). */
_CWIPC_UTIL_EXPORT cwipc_hip_rgbd_rig *cwipc_hip_rgbd_rig_create_decimated(const cwipc_hip_rgbd_sensor *sensors, int ncam, int decimation,
                                                                           char **errorMessage);
/* 1 .. 8; 0 for NULL */
_CWIPC_UTIL_EXPORT int cwipc_hip_rgbd_rig_decimation(const cwipc_hip_rgbd_rig *rig);
/* Camera cam's sensor on the rig's grid -- the derived one of RULE D, the caller's own when decimation == 1 -- with serial = NULL in the
 * copy; 0 ok, -1 for a bad argument. */
_CWIPC_UTIL_EXPORT int cwipc_hip_rgbd_rig_grid_sensor(const cwipc_hip_rgbd_rig *rig, int cam, cwipc_hip_rgbd_sensor *out);
/* One device-resident cloud from one frame (frames: ncam entries, in the sensors' order).  Per camera:
 *  D. Only on a rig made by cwipc_hip_rgbd_rig_create_decimated with decimation > 1 (above, RULE D): the full-size depth image is
 *     replaced by its decimated version, and "the sensor" below is the derived one.
 *  0. Only through cwipc_hip_rgbd_rig_grab_filtered (below, where rules 0a and 0b are stated) and cwipc_hip_rgbd_rig_grab_filled (rule
 *     0c): the depth image is replaced by its spatially and temporally filtered, then hole-filled version.  Rules 1-4 run on that image.
 *  1. Erosion of the depth image (prep may be NULL: none): a pixel keeps its depth iff no pixel (u + du, v + dv) with |du| <=
 *     depth_x_erosion, |dv| <= depth_y_erosion that lies inside the image has depth 0.  Pixels outside the image do not erode.
 *  2. The point of pixel (u, v), depth d != 0:  z = (double)d * depth_scale;  xc = xn*z;  yc = yn*z, (xn, yn) the ray table's entry;
 *     X = ((m00*xc + m01*yc) + m02*z) + m03, Y and Z alike, m = trafo, as cwipc_hip_from_rgbd.  EXCEPTION: a sensor whose eight depth
 *     coefficients are all zero takes xc and yc as cwipc_hip_from_rgbd does: ((u - cx) * z) / fx.
 *  3. Its colour:  P = depth_to_colour . (xc, yc, z), each row ((r0*xc + r1*yc) + r2*z) + r3.  Pz <= 0 or not finite: none.
 *     (x', y') = distort(Px / Pz, Py / Pz) with colour_coeffs;  uc = floor((colour_fx*x' + colour_cx) + 0.5), vc alike; outside
 *     [0, colour_width) x [0, colour_height), tested on the doubles, or NaN: none.  Otherwise the colour of that pixel: the nearest
 *     one.  Occlusion between the two sensors is NOT modelled unless asked for (cwipc_hip_rgbd_rig_grab_occluded below).  A depth
 *     pixel without a ray or without a colour gives no point.
 *  4. The four filters of cwipc_hip_from_rgbd, unchanged, in their order, on the point and that colour; then stable compaction: the
 *     cameras in argument order, the pixels row-major.
 * attach_flags: "depth.<serial>" is the depth image the cloud was made from -- eroded, and 0 where the pixel has no ray or no colour --
 * ("width=W,height=H,bpp=2"), "rgb.<serial>" the colour image REGISTERED onto the depth grid, R, G, B bytes, black where there is
 * none ("width=W,height=H,bpp=3"); per camera rgb then depth.  The images may be ordinary or page-locked memory and are free again on
 * return.  NULL, and nothing left behind, for a NULL rig or frames or image, an erosion outside 0 .. 32, attach_flags with a sensor
 * that has no serial, a rig made on another device than the calling thread's. */
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_rgbd_rig_grab(cwipc_hip_rgbd_rig *rig, const cwipc_hip_rgbd_frame *frames, const cwipc_hip_rgbd_prep *prep,
                                                             const cwipc_hip_rgbd_filter *filter, uint64_t timestamp, float cellsize, int attach_flags,
                                                             char **errorMessage);
/* The same with the occlusion between the two sensors modelled: a z-buffer of every camera's colour grid, as a camera vendor's
 * depth-to-colour transformation has one.  Without it the band of background that the depth sensor sees beside a foreground edge and
 * the colour sensor, a few centimetres to the side, does not, carries the foreground's colour.  This project's own definition, in the
 * notation of rules 1-4 (csrc/rgbd_lens.hpp; tests/rgbd_occlusion_model.py in numpy); float64, every operation rounded on its own:
 *  3a. A depth pixel is a CANDIDATE when it has depth after erosion and rule 3 gives it a colour pixel (uc, vc) -- so it has a ray, and
 *      its Pz is finite and > 0.  Per camera, Zmin(a, b) is the minimum of Pz(q) over the candidates q with |uc(q) - a| <= splat and
 *      |vc(q) - b| <= splat, for the cells (a, b) inside the colour image.
 *  3b. Candidate p is OCCLUDED iff Zmin(uc(p), vc(p)) < Pz(p) - margin (one subtraction, a strict comparison; p is in its own square,
 *      so Zmin <= Pz(p), and equal depths never occlude each other).  An occluded pixel is a pixel without a colour: no point, its depth
 *      cleared and its registered colour black in the attached images.  Then rule 4.
 * splat: 0 .. 8 colour pixels; margin: metres, finite, >= 0.  The colour grid is usually finer than the depth grid, so with splat 0 the
 * foreground's samples leave gaps the background shows through: splat >= ceil(max(colour_fx / fx, colour_fy / fy)) - 1 closes them.  A
 * slanted surface's own neighbours within the splat are nearer than it, which margin must cover (DESIGN 3.19 has the rule of thumb).
 * The result does not depend on the order the minimum is taken in.  occlusion == NULL: cwipc_hip_rgbd_rig_grab, byte for byte.  NULL,
 * and nothing left behind, for a splat outside 0 .. 8, a margin that is negative or not finite, and everything rig_grab refuses.  The
 * z-buffer (8 bytes per colour pixel) is allocated by a rig's first occluded grab and freed with the rig. */
typedef struct cwipc_hip_rgbd_occlusion {
    int32_t splat;
    double margin;
} cwipc_hip_rgbd_occlusion;
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_rgbd_rig_grab_occluded(cwipc_hip_rgbd_rig *rig, const cwipc_hip_rgbd_frame *frames,
                                                                      const cwipc_hip_rgbd_prep *prep, const cwipc_hip_rgbd_occlusion *occlusion,
                                                                      const cwipc_hip_rgbd_filter *filter, uint64_t timestamp, float cellsize,
                                                                      int attach_flags, char **errorMessage);
/* The same with the depth post-processing every depth-camera vendor ships in front of it: an edge-preserving spatial smoother and a
 * temporal smoother that also persists depth over dropped samples.  This project's own definition (the camera plug-ins
 * that hold the vendors' versions are not in the reference tree); csrc/rgbd_depthfilter.hpp is the one statement of the arithmetic,
 * tests/rgbd_depthfilter_model.py its numpy restatement.  RULE 0, in front of rule 1.  All arithmetic is float64, every operation
 * rounded on its own; depth values are in depth units, not metres; oma = 1 - alpha is computed once per call;
 * q(x) = (uint16) floor(x + 0.5).
 *  0a. The spatial filter, spatial_magnitude iterations (0: off, at most 5).  One iteration is, per camera: (1) every row, forward
 *      (u rising); (2) every row, backward, on the result of 1; (3) every column, forward (v rising), on the result of 2; (4) every
 *      column, backward, on the result of 3.  A pass over a line d[0 .. n-1]:
 *          s = (double) d[first]                                    the running value, 0: none
 *          for each further i in pass order:   c = (double) d[i]
 *              if d[i] != 0 and s != 0 and fabs(c - s) < spatial_delta:   s = (spatial_alpha * c) + (oma * s);   d[i] = q(s)
 *              else:                                                      s = c
 *      The comparison is strict and s stays unrounded.  A pixel without depth is never filled and resets the running value; the first
 *      pixel of a pass is never changed by that pass; a line never continues into another row, another column or another camera.  The
 *      new d[i] is a convex combination of two values in 1 .. 65535 and lies there: no clamp is part of the rule.
 *  0b. The temporal filter (temporal 0 / 1), after 0a.  Per depth pixel the rig keeps a running value s (float64, 0: none) and a
 *      history byte h: bit j of h is set iff the pixel had depth -- after 0a, before persistence -- in the j+1-th most recent temporal
 *      grab.  With c the pixel's value after 0a:
 *          if c != 0:   if s != 0 and fabs(c - s) < temporal_delta:   s = (temporal_alpha * c) + (oma_t * s);   out = q(s)
 *                       else:                                         s = c;                                    out = c
 *          else:        out = (s != 0 and persists(temporal_persistency, h)) ? q(s) : 0                         (s unchanged)
 *          h = ((h << 1) | (c != 0)) & 0xff
 *      persists(mode, h), on h as it was before this grab:  0 never;  1 h == 0xff;  2 popcount(h & 0x07) >= 2;
 *      3 popcount(h & 0x0f) >= 2;  4 popcount(h) >= 2;  5 (h & 0x03) != 0;  6 (h & 0x1f) != 0;  7 h != 0;  8 always.
 *      out replaces the depth image: erosion, rays and colour (with occlusion when asked for), then the filters, run on it, and the
 *      attached "depth.<serial>" image is the filtered one, eroded and cleared as before.
 * The state (9 bytes per depth pixel) is allocated by a rig's first grab with temporal != 0 and freed with the rig.  A new rig starts
 * empty (s = 0, h = 0 everywhere); cwipc_hip_rgbd_rig_reset_history makes it empty again.  Only a grab with temporal != 0 reads or
 * writes it; a grab that is refused for its arguments leaves it untouched; a grab that fails on the device leaves it empty.  Grabs
 * are serialised by the rig's lock, which is what gives "the previous grab" a meaning.
 * depthfilter == NULL, or one with spatial_magnitude == 0 and temporal == 0: cwipc_hip_rgbd_rig_grab (occlusion == NULL) or
 * cwipc_hip_rgbd_rig_grab_occluded byte for byte, the history untouched.  NULL, and nothing left behind, for a magnitude outside
 * 0 .. 5, a persistency outside 0 .. 8, and, for a stage that is on, an alpha outside (0, 1] or not finite or a delta that is not
 * finite or not > 0 (the parameters of a stage that is off are not judged), and everything the two other entries refuse. */
typedef struct cwipc_hip_rgbd_depthfilter {
    int32_t spatial_magnitude;                  /* 0 .. 5 iterations, 0: off */
    double spatial_alpha, spatial_delta;        /* 0 < alpha <= 1; delta > 0, depth units; both finite */
    int32_t temporal;                           /* 0 / 1 */
    double temporal_alpha, temporal_delta;      /* as above */
    int32_t temporal_persistency;               /* 0 .. 8 */
} cwipc_hip_rgbd_depthfilter;
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_rgbd_rig_grab_filtered(cwipc_hip_rgbd_rig *rig, const cwipc_hip_rgbd_frame *frames,
                                                                      const cwipc_hip_rgbd_depthfilter *depthfilter, const cwipc_hip_rgbd_prep *prep,
                                                                      const cwipc_hip_rgbd_occlusion *occlusion, const cwipc_hip_rgbd_filter *filter,
                                                                      uint64_t timestamp, float cellsize, int attach_flags, char **errorMessage);
/* The same with HOLE FILLING between rule 0b and rule 1; this project's own definition, stated in csrc/rgbd_decimate.hpp
 * and restated in tests/rgbd_decimate_model.py.  RULE 0c, per camera, on the rig's grid, on the image rules 0a and 0b leave:
 *   mode 1 (from the left):      a pixel without depth takes the value of the nearest pixel WITH depth to its left in the same row; if
 *                                there is none it stays 0.
 *   mode 2 (farthest around):    a pixel without depth takes the largest non-zero value among its up to eight neighbours inside the
 *                                image, read from the stage's INPUT: the fill is not in place, nothing propagates, the result does not
 *                                depend on an order.  If no neighbour has depth it stays 0.
 *   mode 3 (nearest around):     the same with the smallest non-zero value.
 * A pixel that has depth is never changed.  The temporal state (s, h) is what it would be without this stage: rule 0b has run before it
 * and sees the holes.  Modes 2 and 3 use a scratch depth plane (2 bytes per depth pixel), allocated by a rig's first grab that needs
 * it and freed with the rig.  holefill == NULL or mode == 0: cwipc_hip_rgbd_rig_grab_filtered byte for byte, in launches as well.
 * NULL, and nothing left behind (the history untouched), for a mode outside 0 .. 3 and everything cwipc_hip_rgbd_rig_grab_filtered
 * refuses. */
typedef struct cwipc_hip_rgbd_holefill {
    int32_t mode;                               /* 0 off, 1 from the left, 2 farthest around, 3 nearest around */
} cwipc_hip_rgbd_holefill;
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_rgbd_rig_grab_filled(cwipc_hip_rgbd_rig *rig, const cwipc_hip_rgbd_frame *frames,
                                                                    const cwipc_hip_rgbd_holefill *holefill, const cwipc_hip_rgbd_depthfilter *depthfilter,
                                                                    const cwipc_hip_rgbd_prep *prep, const cwipc_hip_rgbd_occlusion *occlusion,
                                                                    const cwipc_hip_rgbd_filter *filter, uint64_t timestamp, float cellsize,
                                                                    int attach_flags, char **errorMessage);
_CWIPC_UTIL_EXPORT void cwipc_hip_rgbd_rig_reset_history(cwipc_hip_rgbd_rig *rig);
/* For parity tests: camera cam's running values (width * height doubles) and history bytes (width * height) into host memory; 0 ok,
 * -1 for a bad argument or a failed copy; a rig without state yet reports zeros. */
_CWIPC_UTIL_EXPORT int cwipc_hip_rgbd_rig_history(cwipc_hip_rgbd_rig *rig, int cam, double *value, uint8_t *history);
/* Camera cam's ray table: 2 * width * height doubles (x then y per pixel, row-major), the rig's own host copy; NULL for a bad argument. */
_CWIPC_UTIL_EXPORT const double *cwipc_hip_rgbd_rig_ray_table(const cwipc_hip_rgbd_rig *rig, int cam);
/* The two mappings for a rig's clouds.  The attached colour image lies on the depth grid, so mapcolordepth is the identity inside the
 * depth image (0 outside) and map2d3d takes depth-grid coordinates: the world point of pixel (u, v) at depth d by rule 2, through the
 * ray table; 0 for a bad argument, (u, v) outside the image, d <= 0, a pixel without a ray. */
_CWIPC_UTIL_EXPORT int cwipc_hip_rgbd_rig_map2d3d(const cwipc_hip_rgbd_rig *rig, int cam, int u, int v, int d, float out[3]);
_CWIPC_UTIL_EXPORT int cwipc_hip_rgbd_rig_mapcolordepth(const cwipc_hip_rgbd_rig *rig, int cam, int u, int v, int out[2]);

/* ---- the octree codec: encoder, encoder group, decoder (csrc/codec_encode.cpp, codec_decode.cpp, codec_host.cpp; csrc/kernels_codec.hip) ----
 * The packets of this codec are NOT interoperable with cwipc_codec: the interface is the reference's (cwipc_new_encoder,
 * cwipc_new_encodergroup, cwipc_new_decoder as python/cwipc/net/sink_encoder.py and source_decoder.py use them), the bitstream is
 * this library's own and carries its own magic.  Out of scope: cwipc_codec's bitstream, JPEG colour coding,
 * per-leaf point counts in the packet, sockets.  (Entropy coding: RULE E below, off unless asked for.  Inter-frame coding: RULE P
 * below, off unless the parameters ask for it; motion compensation is out of scope.  Transform colour coding: RULE T below, off
 * unless asked for.  Level-of-detail decoding and packet thinning: RULE L below, a decoder's choice, off unless asked for; an
 * encoder-side option, thinning a "cwat" or "cwap" packet in one call and an inverse transform that stops early are out of scope.)
 *
 * RULE C.  The arithmetic is csrc/codec_terms.hpp (host and device compile it), tests/codec_model.py its numpy restatement.  All
 * arithmetic is float64 unless stated otherwise, every operation rounded on its own.
 *  Input.   tilenumber != 0: the cloud is first filtered exactly as cwipc_tilefilter(pc, tilenumber) does; voxelsize > 0: then
 *           downsampled exactly as cwipc_downsample(pc, voxelsize) does; then every point with a non-finite coordinate is left out.
 *           What remains, in input order, is P.  An empty P is legal.
 *  Cube.    min_a, max_a: the float32 extremes of P per axis (a zero minimum is +0).  side = max_a(fl64(max_a - min_a)); side == 0: side := 1.
 *  Cell.    For b = octree_bits in 1..16:  u_a = fl64(fl64(p_a - min_a) / side);  q_a = min(2^b - 1, (int) floor(u_a * 2^b)) (the
 *           product is exact).  Hence q_a(b - 1) == q_a(b) >> 1 for every point, at the clamp too (p <= max gives u <= 1).
 *  Key.     3b bits, most significant triple first; within a triple x, y, z with x most significant.  Child index = the triple, 0..7.
 *  Leaves.  The distinct keys in ascending order.  Per leaf over its points: count; per channel m = (sum + count / 2) / count in
 *           integers; tile = OR of the points' tiles.
 *  Colour.  jpeg_quality q gives a shift s: q >= 90: 0; 75..89: 1; 50..74: 2; 25..49: 3; below 25: 4.  Stored: m >> s in 8 - s bits.
 *           Decoded: min(255, (v << s) + ((1 << s) >> 1)).
 *  Packet, little endian, its total length exact:
 *      0  u32 magic, the bytes c w a o        4  u32 version = 1            8  u64 timestamp of the cloud fed
 *     16  u32 nleaves                        20  u8 octree_bits            21  u8 colour bits (8 - s)
 *     22  u8 tile_mode: 0 = all leaves share tile_value, 1 = tile plane present
 *     23  u8 tile_value (0 when mode 1 or nleaves == 0)
 *     24  f32 min_x, min_y, min_z (0 when nleaves == 0)     36  u32 0      40  f64 side (1 when nleaves == 0)
 *     48  u32 nodes[b]: nodes[L] = number of distinct key prefixes of L + 1 triples; nodes[b - 1] == nleaves; all 0 when nleaves == 0
 *     then the occupancy bytes, depth 0 (the root, 1 byte) to depth b - 1, the nodes of a depth in ascending prefix order, bit c set
 *          iff child c exists: 1 + nodes[0] + ... + nodes[b - 2] bytes, absent when nleaves == 0, padded with zeros to a multiple of 4;
 *     then the colours: per leaf r, g, b of 8 - s bits each, leaf-major, packed LSB first into bytes, padded with zeros to a multiple of 4;
 *     then the tile plane: nleaves bytes, only when tile_mode == 1.
 *  Decoding.  One point per leaf in key order: cell = side / 2^b; p_a = (float)(fl64(min_a) + fl64(fl64(q_a + 0.5) * cell)); the colour
 *           by the colour rule, the tile from the tile byte; the cloud's timestamp is the header's, its cellsize (float) cell.
 *  Parameters.  macroblock_size is accepted and ignored.  do_inter_frame == true, gop_size != 1 and exp_factor != 1.0 are refused at
 *           construction (errorMessage plus NULL) unless all three together turn inter mode on (RULE P); so are octree_bits outside
 *           1..16 and jpeg_quality outside 0..100.
 *  Validity.  A packet is valid iff magic, version and ranges are right; nodes[0] <= 8 and nodes[L + 1] <= 8 nodes[L]; no occupancy
 *           byte is 0; the popcounts of depth L sum to nodes[L] (for the last depth: nleaves); padding is 0; the length is exact.
 *           Validation is host code, reads the packet once and runs BEFORE anything is launched or allocated on the device.
 * Results queue first-in first-out per encoder and decoder.  feed returns with the work in flight on the calling thread's stream;
 * available(false) polls, available(true) waits.  No exception crosses this boundary.
 *
 * RULE E, the entropy-coded form.  A packet with the magic "cwae" stands for exactly one valid RULE C packet P ("cwao"):
 * unpack(pack(P)) == P byte for byte, and a decoder fed pack(P) hands out the cloud it hands out for P.  An encoder delivers it only
 * after cwipc_hip_encoder_set_entropy(enc, 1); a decoder takes both forms.  The arithmetic is csrc/entropy_terms.hpp (host and device
 * compile it), tests/entropy_model.py its numpy restatement.  All integers little endian.
 *  Streams.  For nleaves > 0, b = octree_bits, cb = colour bits, in this order: the occupancy bytes of depth 0 .. b - 1 (depth d: 1
 *           symbol for d == 0, nodes[d - 1] otherwise); the leaves' stored colours, one stream per channel r, g, b, nleaves symbols
 *           of cb bits each, carried as byte values; the tile plane, nleaves symbols, only when tile_mode == 1.  S = b + 3 + tile_mode
 *           streams; S = 0 for nleaves == 0.
 *  Prediction.  Colour streams only: symbol j is (v[j] - v[j - 1]) mod 2^cb, and v[j] itself where j mod 4096 == 0.  The decoder undoes
 *           it with an inclusive scan mod 2^cb inside each block.  Occupancy and tile symbols are the bytes themselves.
 *  Blocks.  A stream is cut into blocks of 4096 symbols, the last of m <= 4096.  Symbol j of a block belongs to lane j mod 64 in round
 *           j div 64.  The coder is rANS: per lane a 32-bit state in [2^16, 2^32), 12-bit frequencies (they sum to M = 4096), 16-bit
 *           words.  A block is 64 x u32, the states the decoder starts from, then its W u16 word slots, W even: the words and, when
 *           their number is odd, one padding word 0.  Its size is 256 + 2 W bytes.
 *  Decoder.  cursor = 0.  For each round r = 0 .., first every lane l with j = 64 r + l < m:  slot = x_l & 4095;  s = the symbol with
 *           cum[s] <= slot < cum[s] + f[s] (the largest s with cum[s] <= slot);  x_l = f[s] * (x_l >> 12) + slot - cum[s];  out[j] = s.
 *           Then, in ascending l, every such lane with x_l < 2^16:  x_l = (x_l << 16) | word[cursor++]; a word slot at or past W reads
 *           as 0.  A block is intact iff every one of its 64 start states is at least 2^16, every one of the 64 states is 2^16 at the
 *           end (the lanes that never had a symbol included), no read went past W, and the cursor ends at W, or at W - 1 with the last
 *           slot, the padding word, being 0.
 *  Encoder.  The exact inverse.  All states start at 2^16; rounds from the last to the first, lanes descending within a round; for
 *           symbol s:  if x >= f[s] << 20 (64-bit): emit x & 0xffff, x >>= 16;  then x = (x / f[s]) * 4096 + x % f[s] + cum[s] in
 *           integers.  The block's words are the emitted words in reverse order of emission; at most one per symbol.
 *  Frequencies.  Per stream, from the 256 counts c of its symbols (u32; 64-bit products), total = their sum:  f[i] = 0 where c[i] == 0,
 *           else max(1, (c[i] * 4096) / total);  d = 4096 - sum f;  d > 0: d is added to the symbol of the largest c, the lowest symbol on
 *           ties;  while d < 0: the symbol of the largest f, the lowest on ties, loses 1 (that f is above 1) and d gains 1.  cum is the
 *           exclusive prefix sum of f.
 *  Mode.    A stream is coded (mode 1) iff it has at least 4096 symbols AND its coded payload is strictly smaller than its raw one;
 *           otherwise raw (mode 0).  Raw payload: the occupancy or tile bytes as they are; for a colour channel the plain values (no
 *           prediction) of cb bits each, packed LSB first; padded with zeros to a multiple of 4.  Coded payload: u16 f[256], then
 *           u32 block_bytes[nblocks], then the blocks.
 *  Packet, its total length exact:
 *      0  u32 magic, the bytes c w a e        4  u32 version = 1
 *      8  bytes 8 .. 48 + 4 b of P verbatim (timestamp to nodes[b - 1])
 *     then u32 S, S entries {u32 mode, u32 payload_bytes}, the payloads in stream order.  nleaves == 0: S = 0 and nothing behind it.
 *     Hence len(pack(P)) <= len(P) + 4 + 11 S.
 *  Validity, in two steps.  The container, on the host, BEFORE anything is launched or allocated on the device: magic and version; the
 *           embedded header by RULE C's range and tree rules; S, every mode and every payload size against the counts of the header
 *           (raw: exactly the padded raw size; coded: at least 4096 symbols, a multiple of 4, room for the table and the states of
 *           every block, strictly smaller than the raw size); sum f == 4096, f[0] == 0 for an occupancy stream, f[s] == 0 for s >= 2^cb
 *           for a colour stream; nblocks == ceil(symbols / 4096), every block_bytes a multiple of 4 in [256, 256 + 8192], their sum
 *           the rest of the payload; padding bytes and bits 0, the length exact; raw occupancy streams by RULE C's rules (no byte 0, the
 *           bits of depth d as many as nodes[d]).  Then the coded streams, on the device: every block intact, and for a coded
 *           occupancy stream RULE C's two conditions; the flags reach the host in one wait inside cwipc_hip_decoder_feed, which refuses
 *           the packet with the reason and launches none of the octree decoder's kernels for it.
 *  Bounds.  For ANY payload bytes the decoding kernels (and their host twins) read only inside the packet and write only inside the
 *           header's counts: the slot search stays inside the 256-entry table, a word past the block reads 0 and raises the flag,
 *           every store is below the stream's symbol count.
 *  Encoding runs on the device after the leaves are made: histograms, frequencies, one wave per block, a plan (sizes, modes, offsets,
 *  directory, total) and a gather.  Only then is the size known: feed returns with that work and the copy of four report words in
 *  flight; whoever polls or takes the result first waits for the report and issues the copy of exactly the packet's bytes.
 *
 * RULE P, inter-frame coding.  The arithmetic is csrc/inter_terms.hpp (host and device compile it), tests/inter_model.py its numpy
 * restatement.  All integers little endian; fl32 / fl64: rounded to float32 / float64, every operation on its own.
 *  Parameters.  Inter mode is on iff do_inter_frame == true and 2 <= gop_size <= 65535 and exp_factor is finite in [1, 16].  Each of
 *           the three alone is refused as under RULE C.  cwipc_hip_encodergroup_addencoder refuses inter parameters (a shared sort
 *           for inter encoders is out of scope).
 *  Packets.  An inter-mode encoder delivers only packets with the magic "cwap".  The 32-byte prefix:
 *      0  u32 magic, the bytes c w a p        4  u32 version = 1            8  u32 kind: 0 key, 1 delta
 *     12  u32 gop_index (0 for a key; 1 .. gop_size - 1 for a delta)       16  u64 ref_timestamp (0 for a key)
 *     24  u32 ref_nleaves (0 for a key)      28  u32 0
 *           Key packet: the prefix, then one complete valid "cwao" packet; after cwipc_hip_encoder_set_entropy(enc, 1) that packet's
 *           "cwae" form.  Delta packet: the prefix, then bytes 8 .. 48 of P's RULE C header verbatim (timestamp to side, no nodes[]),
 *           then u32 nadded, then u32 nodesA[b], then u32 S, S entries {u32 mode, u32 payload_bytes}, the payloads.  The length is exact.
 *  Cube of a key frame.  min_a, max_a, side by RULE C.  side' = fl64(side * (double)exp_factor);  margin = fl64(fl64(side' - side) * 0.5);
 *           min'_a = fl32(fl64(fl64(min_a) - margin)), a zero being +0.  The frame is quantised by RULE C's Cell and Key rules in
 *           (min', side'), the clamp included.  With exp_factor == 1 the embedded packet is byte for byte a plain encoder's.
 *  Contained.  A frame with the float32 extremes lo_a, hi_a is contained in (min', side') iff for every axis lo_a >= min'_a and
 *           fl64(fl64(fl64(hi_a) - fl64(min'_a)) / side') <= 1.0.
 *  Sequence.  The encoder holds a counter g (0 at first), the GOP's cube, and a reference R: the frame before as it decodes (keys
 *           ascending, stored colours, tiles), its timestamp and leaf count.  A frame is a key frame iff g == 0, or no reference is
 *           held, or P is empty, or the frame is not contained in the GOP's cube; a key frame forced inside a GOP sets g to 0 first;
 *           a key frame with leaves sets the GOP's cube.  After a frame g = (g + 1) mod gop_size.  An empty P is a key frame (RULE C's
 *           packet of an empty cloud behind the prefix) and leaves no reference.  cwipc_hip_encoder_at_gop_boundary() is true iff
 *           g == 0 or no reference is held.
 *  Delta.   P: the frame's RULE C leaves in the GOP's cube; nR and nleaves are above 0.
 *           keep: ceil(nR / 8) bytes, bit i mod 8 of byte i div 8 set iff R's leaf i is a leaf of P; unused bits 0.
 *           A: the leaves of P that are not in R, nadded of them.  nadded > 0: nodesA[] and A's occupancy bytes by RULE C; otherwise
 *           nodesA is all 0 and there is no occupancy stream.
 *           Predictor of P's leaf j with key k: ub = the number of R keys <= k, pred = max(0, ub - 1): the same leaf where R has it,
 *           otherwise R's predecessor in key order.  Colour symbol per channel: (vP[j] - vR[pred]) mod 2^cb.  Tile symbol, only when
 *           P's tile_mode == 1: tP[j] XOR tR[pred], tR being R's tile_value throughout when R has no tile plane.
 *           Streams, in this order: keep; A's occupancy of depth 0 .. b - 1 (1, nodesA[0], ... symbols); r, g, b of nleaves symbols
 *           each; the tile.  S = 1 + (nadded ? b : 0) + 3 + tile_mode.
 *           Modes, raw and coded payloads, blocks, frequencies and the mode choice are RULE E's, word for word: a stream is coded iff it
 *           has at least 4096 symbols and is strictly smaller coded.  RULE E's colour prediction is NOT applied on top; a raw colour
 *           stream is packed at cb bits; f[0] == 0 is demanded of A's occupancy streams only.
 *  What a delta stands for.  apply(D, R) is exactly one valid "cwao" packet P: its leaves are the merge of the kept R keys and A;
 *           colour (vR[pred] + symbol) mod 2^cb; tile tR[pred] XOR symbol, or tile_value; occupancy and nodes[] rebuilt from the leaves;
 *           the header fields from D.  apply(diff(P, R), R) == P byte for byte, and a decoder fed D after R hands out the cloud it
 *           hands out for P.  Stored values are exact: a chain of deltas does not drift.
 *  Validity, in two steps as in RULE E.  On the host, BEFORE anything is launched or allocated: the prefix, kind and gop_index
 *           (1 .. 65534 for a delta, ref_nleaves > 0); the embedded header's ranges; nleaves > 0; nadded <= nleaves and
 *           nleaves - nadded <= ref_nleaves; nodesA by RULE C's tree rules with nodesA[b - 1] == nadded; S, the modes and the payload
 *           sizes against those counts and ref_nleaves; the tables and block sizes, the padding, the length; raw occupancy streams by
 *           RULE C's rules; for a decoder: a reference is held, and its timestamp, leaf count, b, cb, min bits and side equal the
 *           packet's.  On the device, the flags fetched in one wait: every coded block intact; A's occupancy by RULE C's two
 *           conditions; keep's padding bits 0; popcount(keep) + nadded == nleaves; no key of A is a key of R.  A refused delta launches
 *           none of the point-making kernels and leaves the held reference as it was.
 *  Decoder.  A decoder keeps a reference only after a "cwap" packet (none after one of an empty cloud); "cwao" and "cwae" packets are
 *           decoded as before and neither keep nor disturb one.
 *  Encoding a delta waits twice: once as RULE C does (nodes[], the cube, and with them the choice between key and delta, made on the
 *  device), once for nadded and nodesA[], which size the entropy stage's streams.  Out of scope: sharing inside an encoder group, a
 *  per-frame choice between the delta and the intra form, a constant-stream mode under the coder's 256 bytes of states per block,
 *  motion compensation, interoperability with cwipc_codec.
 *
 * RULE T, transform colour coding (an integer region-adaptive hierarchical transform, RAHT).  A packet with the magic "cwat" stands
 * for exactly one valid RULE C packet with 8 colour bits: unpack(T) has T's header, occupancy and tiles and the colours the inverse
 * transform gives, and a decoder fed T hands out the cloud it hands out for unpack(T).  pack(P, quality) is a function of a valid
 * 8-bit "cwao" packet P and the quality; unpack(pack(P, 100)) == P byte for byte.  An encoder delivers it only after
 * cwipc_hip_encoder_set_colour_transform(enc, 1).  The arithmetic is csrc/transform_terms.hpp (host and device compile it),
 * tests/transform_model.py its numpy restatement.  Integers only, little endian; >> is an arithmetic shift; / on non-negative values
 * truncates; floor() rounds towards minus infinity.
 *  Input.   The leaves of RULE C as the same encoder makes them with s = 0: keys ascending, the 8-bit rounded means m, tiles.  The
 *           header's colour bits are 8.  jpeg_quality selects the quantiser, not a shift.
 *  Scale.   q = max(1, jpeg_quality);  sc = q < 50 ? 5000 / q : 200 - 2 q;  Q16 = min(1024, 16 + (12 sc) / 10).  Q16 travels in the
 *           packet (100 gives 16, 85: 52, 50: 136, 25: 256, 1 and 0: 1024); a decoder never sees jpeg_quality.
 *  Colour.  Per leaf, reversible YCoCg-R:  Co = R - B;  t = B + (Co >> 1);  Cg = G - t;  Y = t + (Cg >> 1).  Back:  t = Y - (Cg >> 1);
 *           G = Cg + t;  B = t - (Co >> 1);  R = B + Co;  then every channel is clamped to 0..255.  The channel scale Q16c is Q16 for
 *           Y and min(1024, 2 Q16) for Co and Cg; at Q16 == 16 it is 16 for all three.
 *  Tree.    A node's weight is the number of leaves beneath it, a leaf's is 1.  A parent merges its present children in three stages
 *           over the child index c = 4x + 2y + z: stage z pairs (c, c ^ 1); stage y pairs the results of (0,1) with (2,3) and of (4,5)
 *           with (6,7); stage x pairs the two halves.  A pair with one side empty passes the other side through, value and weight.
 *           A pair with both sides present is a butterfly of (a, w1), the side of the lower index, and (b, w2);  W = w1 + w2:
 *           d = b - a;  l = a + floor((w2 d + (W >> 1)) / W) in 64 bits;  the merged node has the value l and the weight W.
 *           A parent of k children yields k - 1 coefficients d; a channel has nleaves - 1 of them and the root's l as dc.
 *  Step.    Of a butterfly, in unsigned 64 bits:  t = (Q16c Q16c (w1 + w2)) / (w1 w2);  step = max(1, (isqrt(t) + 8) >> 4), isqrt the
 *           exact floor of the square root.  (RAHT's sqrt(w1 w2 / (w1 + w2)) folded into the step.)  Q16c == 16 gives step 1 throughout.
 *  Quantiser.  c = sign(d) ((|d| + step / 2) / step);  reconstructed d^ = c step.  The encoder is open loop: it quantises the exact d.
 *  Inverse.  From dc down.  A butterfly with its l^:  a^ = l^ - floor((w2 d^ + (W >> 1)) / W);  b^ = a^ + d^.  Nothing is clamped
 *           inside the tree.  With step 1 everywhere the inverse is exact.
 *  Order.   Of the coefficients of a channel: by the depth of the parent, the root first; the parents of a depth in ascending prefix
 *           order; within a parent the x butterfly, then the y butterflies (low half first), then the z butterflies in ascending c,
 *           those that exist.  (With the nodes numbered across depths, root 0, a parent i whose first child is s has its first
 *           coefficient at s - i - 1.)
 *  Symbols.  zz = c >= 0 ? 2 c : -2 c - 1;  token = min(zz, 255);  a coefficient with zz >= 255 also appends zz - 255 as a u16 to its
 *           channel's escape stream, in coefficient order (the encoder's |d| is at most 510, so zz - 255 fits).
 *  Streams, in this order: the occupancy bytes of depth 0 .. b - 1 as in RULE E; for Y, Co, Cg in turn the token stream (nleaves - 1
 *           symbols) and then the escape stream; the tile plane when tile_mode == 1.  S = b + 6 + tile_mode, 0 for nleaves == 0.
 *           Token, occupancy and tile streams take RULE E's modes, blocks, frequencies and mode choice word for word (coded iff at
 *           least 4096 symbols and strictly smaller coded); nothing is predicted.  An escape stream is always raw: its u16 values,
 *           padded with zeros to a multiple of 4.  A stream without symbols has mode 0 and an empty payload.
 *  Packet, its total length exact:
 *      0  u32 magic, the bytes c w a t        4  u32 version = 1
 *      8  bytes 8 .. 48 + 4 b of the RULE C packet verbatim (colour bits 8)
 *     then u16 Q16, i16 dc[3] (Y, Co, Cg), u32 nescapes[3], then u32 S, S entries {u32 mode, u32 payload_bytes}, the payloads.
 *     nleaves == 0: dc and nescapes are 0, S = 0 and nothing behind it.
 *  Validity, in two steps as in RULE E.  On the host, BEFORE anything is launched or allocated: magic, version, the embedded header by
 *           RULE C's range and tree rules with colour bits == 8; 16 <= Q16 <= 1024; nescapes[i] <= nleaves - 1 (0 and dc 0 for an
 *           empty cloud); S, every mode (an escape stream's is 0) and payload size against the header's counts and nescapes; tables,
 *           block sizes, padding, the length; raw occupancy streams by RULE C's rules.  On the device, fetched in the one wait inside
 *           cwipc_hip_decoder_feed: every coded block intact; coded occupancy by RULE C's two conditions; per channel the number of
 *           tokens equal to 255 is nescapes[i].  A refused packet launches none of the point-making kernels.
 *  Bounds.  For ANY payload bytes zz <= 255 + 65535, so |d^| <= 32895 * 91, and at most 3 b additions of it and 1 reach a leaf from
 *           dc: every value stays far inside 32 bits, every product inside 64.  Every load is inside the packet or the tree's node
 *           count, every store below the header's counts.
 *  Parameters.  cwipc_hip_encoder_set_colour_transform is legal before the first feed and implies RULE E's container for geometry and
 *           tiles.  An inter-mode encoder refuses it: a delta's colour differences are exact residuals to the reference, and a lossy
 *           transform under RULE P needs a design of its own.  An encoder of a group may have it on.
 *  Header's choices (the rule's text left them open): version 1 shares RULE C's version test; a packet of one leaf has three token
 *           streams without symbols; the escape streams' directory entries count their padded bytes; Q16 of an empty cloud's packet is
 *           the quality's.  Out of scope: transform colour under RULE P, per-depth frequency tables or contexts, a constant-stream
 *           mode under the coder's 256 bytes of states per block, prediction between levels, closed-loop quantisation, per-leaf point
 *           counts as weights, interoperability with cwipc_codec or G-PCC.
 *
 * RULE L, level-of-detail cuts.  By RULE C's cell rule q_a(b - 1) == q_a(b) >> 1, so the first t triples of a b-bit key are the key of
 * the same point at t bits: a packet's first t depths ARE the geometry of the same cloud coded at t bits.  The arithmetic is
 * csrc/lod_terms.hpp (host and device compile it), tests/lod_model.py its numpy restatement.  Integers only.
 *  For a valid "cwao" packet P with b octree bits, cb colour bits and nleaves > 0, and a target t with 1 <= t < b, L(P, t) is the
 *  "cwao" packet with:
 *  Header.  timestamp, min, side and cb as P's; octree_bits = t; nodes' = nodes[0 .. t - 1]; nleaves' = nodes[t - 1].
 *  Occupancy.  The occupancy bytes of depths 0 .. t - 1 verbatim, padded anew.
 *  Colours.  One leaf per distinct key prefix of t triples, ascending.  A new leaf's members are P's leaves under it: a contiguous run
 *           of n >= 1 leaves in key order.  Per channel on the STORED values (cb bits): v' = (sum v + n / 2) div n in integers.  The
 *           sum is exact for any n up to nleaves: it is kept in 64 bits.
 *  Tiles.   tile' = OR of the members' tiles (tile_value for all of them when P has tile_mode 0).  tile_mode' and tile_value' are decided
 *           anew by the encoder's rule: mode 0 iff all new leaves share one value.  A tile plane can therefore disappear.
 *  Fixed points and limits.  L(P, b) == P byte for byte, whatever P's tile mode.  An empty P maps to RULE C's empty packet of t bits
 *           with P's timestamp and colour bits.  t < 1 and t > b are refused by the packet function; for a decoder t >= b means the
 *           packet as it is.
 *  Not promised.  L(L(P, t), u) == L(P, u): those are means of means.  Equality of L(P, t)'s colours with those of the same cloud
 *           encoded at t bits: that encode takes its means over points, and a packet holds no point counts.  Everything but the
 *           colours IS equal: bytes 24 .. 48, nodes', the occupancy section, nleaves' and the tile fields and plane.
 *  Decoder.  cwipc_hip_decoder_set_max_octree_bits(dec, bits): for a packet that stands for a "cwao" packet P with b > bits the decoder
 *           hands out exactly the cloud that decoding L(P, bits) gives: points, colours, tiles, timestamp, cellsize = side / 2^bits.
 *           "cwat": L applies to the 8-colour-bit packet it stands for, the inverse transform runs in full.  "cwap": the reference the
 *           decoder keeps stays the FULL frame, so chains do not drift and later deltas validate as before; only the cloud handed
 *           out is cut.  Every validity test and refusal is as without the setting and comes before any kernel of csrc/kernels_lod.hip.
 *  Out of scope.  Thinning "cwat" or "cwap" packets in one call (compose with their unpack functions); an inverse transform that stops
 *           early (RULE T's low-pass values are weighted, they are not RULE L's colours); point counts in packets; an encoder-side
 *           option; any change to RULES C, E, P, T or their packets. */
typedef struct cwipc_hip_encoder_params {
    bool do_inter_frame;     /* false; true with the two below: inter mode (RULE P) */
    int gop_size;            /* 1; inter mode: 2..65535 */
    float exp_factor;        /* 1.0; inter mode: 1.0..16.0 */
    int octree_bits;         /* 1..16 */
    int jpeg_quality;        /* 0..100: the colour shift; with RULE T on: the quantiser scale */
    int macroblock_size;     /* accepted and ignored */
    int tilenumber;          /* 0: every point */
    float voxelsize;         /* > 0: cwipc_downsample first */
} cwipc_hip_encoder_params;
typedef struct cwipc_hip_encoder cwipc_hip_encoder;
typedef struct cwipc_hip_encodergroup cwipc_hip_encodergroup;
typedef struct cwipc_hip_decoder cwipc_hip_decoder;
_CWIPC_UTIL_EXPORT cwipc_hip_encoder *cwipc_hip_new_encoder(const cwipc_hip_encoder_params *params, char **errorMessage);
_CWIPC_UTIL_EXPORT void cwipc_hip_encoder_free(cwipc_hip_encoder *enc);
_CWIPC_UTIL_EXPORT int cwipc_hip_encoder_feed(cwipc_hip_encoder *enc, cwipc_pointcloud *pc);        /* 0 ok, -1 error (logged) */
/* on != 0: the encoder delivers RULE E's entropy-coded form ("cwae") of the packets it would deliver otherwise.  Legal before the first
 * feed, also on an encoder of a group (the group's sort is shared all the same); afterwards -1 and the reason in cwipc_hip_last_error(). */
_CWIPC_UTIL_EXPORT int cwipc_hip_encoder_set_entropy(cwipc_hip_encoder *enc, int on);
/* on != 0: the encoder delivers RULE T's transform-coded form ("cwat"): colours at 8 bits through the integer transform, quantised by
 * jpeg_quality; geometry and tiles as under RULE E.  Legal before the first feed, also on an encoder of a group; -1 and the reason in
 * cwipc_hip_last_error() afterwards, and for an inter-mode encoder. */
_CWIPC_UTIL_EXPORT int cwipc_hip_encoder_set_colour_transform(cwipc_hip_encoder *enc, int on);
_CWIPC_UTIL_EXPORT bool cwipc_hip_encoder_available(cwipc_hip_encoder *enc, bool wait);
_CWIPC_UTIL_EXPORT size_t cwipc_hip_encoder_get_encoded_size(cwipc_hip_encoder *enc);               /* of the oldest result; 0: none */
_CWIPC_UTIL_EXPORT bool cwipc_hip_encoder_copy_data(cwipc_hip_encoder *enc, void *buffer, size_t size);   /* takes the oldest result */
_CWIPC_UTIL_EXPORT bool cwipc_hip_encoder_at_gop_boundary(cwipc_hip_encoder *enc);                   /* RULE P; always true without inter mode */
_CWIPC_UTIL_EXPORT bool cwipc_hip_encoder_eof(cwipc_hip_encoder *enc);                               /* closed and nothing queued */
_CWIPC_UTIL_EXPORT void cwipc_hip_encoder_close(cwipc_hip_encoder *enc);
_CWIPC_UTIL_EXPORT cwipc_hip_encodergroup *cwipc_hip_new_encodergroup(char **errorMessage);
/* The new encoder belongs to the group (freed with it).  feed: every encoder of the group receives what it would deliver alone, byte
 * for byte; encoders with equal (tilenumber, voxelsize) share one filtered cloud and one sort, made at their largest octree_bits. */
_CWIPC_UTIL_EXPORT cwipc_hip_encoder *cwipc_hip_encodergroup_addencoder(cwipc_hip_encodergroup *group, const cwipc_hip_encoder_params *params,
                                                                        char **errorMessage);
_CWIPC_UTIL_EXPORT int cwipc_hip_encodergroup_feed(cwipc_hip_encodergroup *group, cwipc_pointcloud *pc);
_CWIPC_UTIL_EXPORT void cwipc_hip_encodergroup_close(cwipc_hip_encodergroup *group);
_CWIPC_UTIL_EXPORT void cwipc_hip_encodergroup_free(cwipc_hip_encodergroup *group);
_CWIPC_UTIL_EXPORT cwipc_hip_decoder *cwipc_hip_new_decoder(char **errorMessage);
/* 0 ok; -1 and the reason in cwipc_hip_last_error() for a packet that is not valid (nothing launched, nothing allocated) or a device failure */
_CWIPC_UTIL_EXPORT int cwipc_hip_decoder_feed(cwipc_hip_decoder *dec, const void *bytes, size_t len);
/* RULE L: the most octree bits of a cloud handed out.  bits 0: off, the default; 1..16: packets of more bits give the cloud of their cut;
 * anything else: -1 and the reason in cwipc_hip_last_error().  Callable between feeds; it applies to later feeds. */
_CWIPC_UTIL_EXPORT int cwipc_hip_decoder_set_max_octree_bits(cwipc_hip_decoder *dec, int bits);
_CWIPC_UTIL_EXPORT bool cwipc_hip_decoder_available(cwipc_hip_decoder *dec, bool wait);
_CWIPC_UTIL_EXPORT cwipc_pointcloud *cwipc_hip_decoder_get(cwipc_hip_decoder *dec);                  /* device-resident; NULL: none */
_CWIPC_UTIL_EXPORT bool cwipc_hip_decoder_eof(cwipc_hip_decoder *dec);
_CWIPC_UTIL_EXPORT void cwipc_hip_decoder_close(cwipc_hip_decoder *dec);
_CWIPC_UTIL_EXPORT void cwipc_hip_decoder_free(cwipc_hip_decoder *dec);
/* A packet's header after the validity test, without a GPU: 0 and *info filled, or -1 and the reason in *errorMessage. */
typedef struct cwipc_hip_codec_info {
    uint64_t timestamp;
    uint32_t nleaves;
    int32_t octree_bits, colour_bits, tile_mode, tile_value;
    float min[3];
    double side;
    uint32_t nodes[16];
    uint64_t occupancy_offset, colour_offset, tile_offset, total_bytes;
} cwipc_hip_codec_info;
_CWIPC_UTIL_EXPORT int cwipc_hip_codec_packet_info(const void *bytes, size_t len, cwipc_hip_codec_info *info, char **errorMessage);
/* RULE E on the host, without a GPU.  pack: a valid "cwao" packet -> its "cwae" form; unpack: a "cwae" packet -> the "cwao" packet it
 * stands for, after the container test, the blocks' integrity and the occupancy rules.  Both return the size of the result and write it
 * to out iff out != NULL and it fits capacity (pack never needs more than len + 4 + 11 * 20 bytes; unpack needs
 * cwipc_hip_codec_entropy_info()'s packet.total_bytes); 0 and the reason in *errorMessage for a packet that is refused. */
_CWIPC_UTIL_EXPORT size_t cwipc_hip_codec_entropy_pack(const void *bytes, size_t len, void *out, size_t capacity, char **errorMessage);
_CWIPC_UTIL_EXPORT size_t cwipc_hip_codec_entropy_unpack(const void *bytes, size_t len, void *out, size_t capacity, char **errorMessage);
/* The directory of a "cwae" packet after the container test (the coded blocks are not decoded): 0 and *info filled, or -1 and the reason. */
typedef struct cwipc_hip_codec_entropy_directory {
    cwipc_hip_codec_info packet;      /* the header; offsets and total_bytes are those of the "cwao" packet it stands for */
    int32_t nstreams;                 /* S */
    int32_t kind[20];                 /* 0 occupancy, 1 colour, 2 tile */
    int32_t which[20];                /* occupancy: the depth; colour: the channel */
    int32_t mode[20];                 /* 0 raw, 1 coded */
    uint32_t symbols[20];
    uint64_t payload_offset[20], payload_bytes[20];
    uint64_t total_bytes;             /* of the "cwae" packet */
} cwipc_hip_codec_entropy_directory;
_CWIPC_UTIL_EXPORT int cwipc_hip_codec_entropy_info(const void *bytes, size_t len, cwipc_hip_codec_entropy_directory *info, char **errorMessage);
/* RULE L on the host, without a GPU: a valid "cwao" packet P -> L(P, bits); a "cwae" packet Q -> entropy_pack(L(entropy_unpack(Q), bits)).
 * "cwat" and "cwap" packets are refused (compose with cwipc_hip_codec_transform_unpack / cwipc_hip_codec_inter_unpack), and so are bits < 1
 * and bits above the packet's.  The caller-buffer convention is cwipc_hip_codec_entropy_pack's; a "cwao" result never needs more than
 * len bytes, a "cwae" result's size comes from a first call with out == NULL. */
_CWIPC_UTIL_EXPORT size_t cwipc_hip_codec_lod(const void *bytes, size_t len, int bits, void *out, size_t capacity, char **errorMessage);
/* RULE T on the host, without a GPU.  pack: a valid "cwao" packet with 8 colour bits and a jpeg_quality in 0..100 -> its "cwat" form
 * (never more than 3 * len + 300 bytes); unpack: a "cwat" packet -> the "cwao" packet it stands for, after the container test, the blocks'
 * integrity, the occupancy rules and the escape counts (cwipc_hip_codec_transform_info()'s packet.total_bytes).  The caller-buffer
 * convention is cwipc_hip_codec_entropy_pack's. */
_CWIPC_UTIL_EXPORT size_t cwipc_hip_codec_transform_pack(const void *bytes, size_t len, int jpeg_quality, void *out, size_t capacity, char **errorMessage);
_CWIPC_UTIL_EXPORT size_t cwipc_hip_codec_transform_unpack(const void *bytes, size_t len, void *out, size_t capacity, char **errorMessage);
/* A "cwat" packet after the container test (the coded blocks are not decoded, the tokens not counted): 0 and *info filled, or -1 and the reason. */
typedef struct cwipc_hip_codec_transform_directory {
    cwipc_hip_codec_info packet;      /* the header; offsets and total_bytes are those of the "cwao" packet it stands for */
    uint32_t q16;
    int32_t dc[3];                    /* Y, Co, Cg */
    uint32_t nescapes[3];
    int32_t nstreams;                 /* S */
    int32_t kind[23];                 /* 0 occupancy, 2 tile, 3 tokens, 5 escapes */
    int32_t which[23];                /* occupancy: the depth; tokens and escapes: the channel */
    int32_t mode[23];                 /* 0 raw, 1 coded */
    uint32_t symbols[23];
    uint64_t payload_offset[23], payload_bytes[23];
    uint64_t total_bytes;             /* of the "cwat" packet */
} cwipc_hip_codec_transform_directory;
_CWIPC_UTIL_EXPORT int cwipc_hip_codec_transform_info(const void *bytes, size_t len, cwipc_hip_codec_transform_directory *info, char **errorMessage);
/* RULE P on the host, without a GPU.  pack: two valid "cwao" packets R and P with leaves, in one cube -> the delta packet diff(P, R);
 * unpack: R and a "cwap" packet -> the "cwao" packet it stands for after all of RULE P's tests (a key packet: its embedded packet
 * verbatim, R may be NULL).  The caller-buffer convention is cwipc_hip_codec_entropy_pack's; pack never needs more than
 * plen + rlen / 8 + 256 bytes, unpack's size comes from a first call with out == NULL. */
_CWIPC_UTIL_EXPORT size_t cwipc_hip_codec_inter_pack(const void *r, size_t rlen, const void *p, size_t plen, uint32_t gop_index, void *out, size_t capacity,
                                                     char **errorMessage);
_CWIPC_UTIL_EXPORT size_t cwipc_hip_codec_inter_unpack(const void *r, size_t rlen, const void *d, size_t dlen, void *out, size_t capacity, char **errorMessage);
/* A "cwap" packet after the container test (the coded blocks are not decoded): 0 and *info filled, or -1 and the reason. */
typedef struct cwipc_hip_codec_inter_directory {
    uint32_t kind, gop_index;         /* the prefix */
    uint64_t ref_timestamp;
    uint32_t ref_nleaves;
    int32_t embedded_entropy;         /* key: the embedded packet is a "cwae" packet */
    cwipc_hip_codec_info packet;      /* the header; key: of the embedded packet's "cwao" form; delta: nodes[], offsets and total_bytes are 0 */
    uint32_t nadded, nodes_added[16];
    int32_t nstreams;                 /* S; 0 for a key packet */
    int32_t kind_of[21];              /* 0 A's occupancy, 3 bytes (keep: which 0, tile: which 1), 4 a colour residual */
    int32_t which[21];
    int32_t mode[21];
    uint32_t symbols[21];
    uint64_t payload_offset[21], payload_bytes[21];
    uint64_t total_bytes;
} cwipc_hip_codec_inter_directory;
_CWIPC_UTIL_EXPORT int cwipc_hip_codec_inter_info(const void *bytes, size_t len, cwipc_hip_codec_inter_directory *info, char **errorMessage);

/* ---- intermediate results for parity tests ---- */
/* Steps 1 to 3 of cwipc_hip_detect_markers: labels (height*width words) receives every dark pixel's component label, -1 for a light
 * pixel; 0 ok, -1 error (the image and parameter checks of cwipc_hip_detect_markers). */
_CWIPC_UTIL_EXPORT int cwipc_hip_marker_labels(const uint8_t *rgb, int width, int height, const cwipc_hip_marker_params *params, int32_t *labels);
/* Mean k-NN distance d_i of every point (the quantity pcl::StatisticalOutlierRemoval thresholds) into host memory; 0 ok. */
_CWIPC_UTIL_EXPORT int cwipc_hip_knn_mean_dist(cwipc_pointcloud *pc, int kNeighbors, float *mean_dist, size_t cap, double *threshold, float stddevMulThresh);
/* The direction filter's normals, in their final orientation, as three planes of cap floats (x then y then z), the size of every
 * point's neighbourhood into nn_count (cap words, may be NULL) and the centroid into centroid (3 floats, may be NULL); 0 ok, -1 error.
 * normals and nn_count both NULL: the centroid alone (the mean of the points, summed in f64; cwipc_center). */
_CWIPC_UTIL_EXPORT int cwipc_hip_estimate_normals(cwipc_pointcloud *pc, float radius, int max_nn, float *normals, uint32_t *nn_count, float *centroid, size_t cap);

/* ---- per-kernel device timing (hipEvents on the calling thread's stream) ---- */
_CWIPC_UTIL_EXPORT void cwipc_hip_profile_enable(int on);
_CWIPC_UTIL_EXPORT void cwipc_hip_profile_reset(void);
/* Number of distinct kernels seen; name/total milliseconds/launch count of entry i. */
_CWIPC_UTIL_EXPORT int cwipc_hip_profile_count(void);
_CWIPC_UTIL_EXPORT int cwipc_hip_profile_get(int i, const char **name, double *total_ms, long *launches);

#ifdef __cplusplus
}
#endif
#endif
