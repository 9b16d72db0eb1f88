/*
 * dvslam_hip.h — C-ABI of libdvslam_hip.so: MI355X (gfx950) implementation of the data-parallel hot
 * path of andrewkwolek/dynamic-visual-slam.  Plain pointers and sizes only; no C++/torch types.
 *
 * The reference has no FFI/plugin layer: its hot path is reached through three C++ call signatures
 * (SURVEY.md §8b).  Each group of entry points below replaces one of them; header-only C++ adapters
 * with the reference's own signatures live in include/dvslam/ (see INTEGRATION.md).
 *
 *   B1  ORB_SLAM3::ORBextractor::ORBextractor / operator()   include/dynamic_visual_slam/ORBextractor.hpp:50-60,
 *                                                            src/ORBextractor.cpp:409-469, 1086-1167
 *   B2  cv::BFMatcher(NORM_HAMMING).match call sites          src/frontend.cpp:220,614,1123; src/backend.cpp:222,1072
 *   B3  SlidingWindowBA / WeightedSquaredReprojectionError    include/dynamic_visual_slam/bundle_adjustment.hpp:469-593, 652-904
 *
 * Conventions: every function returns a dvs_status (0 = ok, < 0 = error; dvs_last_error() gives text);
 * nothing is allocated across the ABI — callers supply output buffers with explicit capacities;
 * a handle owns one HIP stream and is not thread-safe, distinct handles are independent.
 * "host" entry points take host pointers (they stage through pinned memory); "_device" entry points
 * take pointers into the handle's GPU memory space and only enqueue work on the handle's stream.
 */
#ifndef DVSLAM_HIP_H
#define DVSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t dvs_status;
enum {
  DVS_OK = 0,
  DVS_ERR_EMPTY = -1,        /* empty image: ORBextractor::operator() returns -1 (ORBextractor.cpp:1090-1091) */
  DVS_ERR_UNSUPPORTED = -2,  /* image size / parameters for which the reference divides by zero (nCols, nIni == 0) */
  DVS_ERR_CAPACITY = -3,     /* caller buffer too small */
  DVS_ERR_HIP = -4,          /* HIP runtime error (message in dvs_last_error) */
  DVS_ERR_NO_DEVICE = -5,    /* no gfx950 device visible: there is NO CPU fallback */
  DVS_ERR_ARG = -6           /* null pointer / negative size / bad enum */
};

const char* dvs_last_error(void);
int32_t dvs_device_count(void);
/* A plain HIP stream for the caller's side work (e.g. the multi-GPU boundary exchange), created by this library so that it
 * can be made right after the handles: HIP maps streams to hardware queues in creation order, and the path's concurrent
 * streams should be neighbours in that order ("Streams and hardware queues"). */
dvs_status dvs_stream_create(int32_t device, int32_t high_priority, void** out_stream);
dvs_status dvs_stream_synchronize(void* stream);
dvs_status dvs_stream_destroy(void* stream);
/* hipEvent_t helpers for callers without a HIP toolchain of their own (the scheduling hooks dvs_orb_set_after_fast_event /
 * dvs_orb_set_output_event take any hipEvent_t): create (timing disabled), destroy, host wait, record, stream wait */
dvs_status dvs_event_create(int32_t device, void** out_event);
dvs_status dvs_event_destroy(void* event);
dvs_status dvs_event_synchronize(void* event);
dvs_status dvs_event_create_timing(int32_t device, void** out_event);   /* an event that records a time stamp */
dvs_status dvs_event_elapsed_ms(void* start, void* stop, float* ms);    /* both created with _create_timing and completed */
dvs_status dvs_event_query(void* event, int32_t* done);   /* *done = 1 when everything recorded before the event has completed */
dvs_status dvs_event_record(void* event, void* stream);
dvs_status dvs_stream_wait_event(void* stream, void* event);
/* "gfx950" etc. for the given device, "" on error */
dvs_status dvs_device_arch(int32_t device, char* buf, int32_t cap);

/* ---- device memory / stream helpers so non-HIP hosts (tests, bench) can stay resident in HBM ---- */
dvs_status dvs_malloc(int32_t device, size_t bytes, void** out);
dvs_status dvs_free(int32_t device, void* p);
dvs_status dvs_memcpy_h2d(int32_t device, void* dst, const void* src, size_t bytes);
dvs_status dvs_memcpy_d2h(int32_t device, void* dst, const void* src, size_t bytes);
dvs_status dvs_memset(int32_t device, void* dst, int value, size_t bytes);

/* ======================================= B1: ORB extractor ===================================== */

typedef struct dvs_orb dvs_orb;

/* same field order and size (28 B) as cv::KeyPoint */
typedef struct dvs_keypoint {
  float x, y;       /* level-0 pixel coordinates (level coords * mvScaleFactor[octave], ORBextractor.cpp:1148-1150) */
  float size;       /* (int)(31 * mvScaleFactor[octave]) (ORBextractor.cpp:880,889) */
  float angle;      /* degrees in [0,360), intensity-centroid orientation (ORBextractor.cpp:76-103) */
  float response;   /* FAST-9/16 corner score */
  int32_t octave;   /* pyramid level */
  int32_t class_id; /* -1 */
} dvs_keypoint;

typedef struct dvs_orb_params {
  int32_t nfeatures;        /* ORBextractor ctor arg 1 (frontend.cpp:206: 1000) */
  float scale_factor;       /* arg 2 (1.2f) */
  int32_t nlevels;          /* arg 3 (8); 1..DVS_MAX_LEVELS */
  int32_t ini_th_fast;      /* arg 4 (20) */
  int32_t min_th_fast;      /* arg 5 (7) */
  int32_t gauss_kernel[7];  /* Q8 7-tap kernel of cv::GaussianBlur(7x7, sigma 2); all zeros = {18,34,48,56,48,34,18} */
  int32_t max_batch;        /* frames processed per launch sequence; 0 = 1 */
} dvs_orb_params;

#define DVS_MAX_LEVELS 16

dvs_status dvs_orb_create(const dvs_orb_params* params, int32_t device, dvs_orb** out);
void dvs_orb_destroy(dvs_orb* h);
/* capacity a caller must provide per frame: nfeatures + 3 * nlevels (a level may return quota + 2, ORBextractor.cpp:746-747) */
int32_t dvs_orb_max_keypoints(const dvs_orb* h);
/* enqueue on a caller-owned hipStream_t (e.g. torch's current stream) instead of the handle's own non-blocking
 * stream; NULL selects HIP's legacy default stream. */
dvs_status dvs_orb_set_stream(dvs_orb* h, void* hip_stream);
void* dvs_orb_get_stream(dvs_orb* h);
dvs_status dvs_orb_synchronize(dvs_orb* h);

/* float tables of the ctor (ORBextractor.cpp:414-445, 451-468); arrays of nlevels (umax: 16) entries, any may be NULL */
dvs_status dvs_orb_get_tables(const dvs_orb* h, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                              int32_t* features_per_level, int32_t* umax16);
dvs_status dvs_orb_level_size(const dvs_orb* h, int32_t rows, int32_t cols, int32_t level, int32_t* level_rows, int32_t* level_cols);

/* operator(): host image (8UC1, `step` bytes between rows) -> host keypoints + N x 32 descriptors.  *n_out = N. */
dvs_status dvs_orb_extract(dvs_orb* h, const uint8_t* gray, int32_t rows, int32_t cols, size_t step,
                           dvs_keypoint* kps, uint8_t* desc, int32_t capacity, int32_t* n_out);
/* nimg host images of identical size; outputs are [nimg][capacity] blocks, n_out[nimg] */
dvs_status dvs_orb_extract_batch(dvs_orb* h, const uint8_t* const* imgs, int32_t nimg, int32_t rows, int32_t cols, size_t step,
                                 dvs_keypoint* kps, uint8_t* desc, int32_t capacity, int32_t* n_out);
/* device-resident batch: frame f starts at d_imgs + f * frame_stride.  Asynchronous on the handle's stream. */
dvs_status dvs_orb_extract_batch_device(dvs_orb* h, const uint8_t* d_imgs, int32_t nimg, int32_t rows, int32_t cols,
                                        size_t step, size_t frame_stride, dvs_keypoint* d_kps, uint8_t* d_desc,
                                        int32_t capacity, int32_t* d_n_out);
/* ---- keep masks (INTEGRATION.md §B1 "Keep masks"): drop corners on dynamic regions before the quad-tree shares out the quotas ----
 * A mask is 8-bit, level-0 sized (rows x cols, `mask_step` bytes between rows), nonzero = keep, as in OpenCV.  A FAST candidate of
 * level l at region-relative (cx, cy) is kept iff mask[min(rows-1, floor(Y))][min(cols-1, floor(X))] != 0 with
 * X = (float)(cx + 16) * mvScaleFactor[l] (Y alike): the coordinates the keypoint would carry, so no output keypoint lies on a masked
 * pixel.  Per-cell FAST (threshold 20, else 7), the quotas, the quad-tree, orientation, blur and descriptors are unchanged: a cell
 * whose threshold-20 corners are all masked does NOT fall back to threshold 7.  An all-nonzero mask gives the unmasked result bit for
 * bit, an all-zero one 0 keypoints.  A NULL mask (masks array) is exactly the unmasked entry point; mask_step < cols is DVS_ERR_ARG.
 * After a masked call the candidate hook (dvs_orb_get_candidates) returns the filtered lists.
 * Not offered: masks for dvs_pipeline_* and the level-sharded dvs_orb_extract_levels_device, dvslam::ORB (OpenCV resizes the mask
 * per level: other semantics), box lists, and skipping FAST on fully masked cells. */
dvs_status dvs_orb_extract_masked(dvs_orb* h, const uint8_t* gray, int32_t rows, int32_t cols, size_t step, const uint8_t* mask, size_t mask_step,
                                  dvs_keypoint* kps, uint8_t* desc, int32_t capacity, int32_t* n_out);
/* masks[nimg] host masks (NULL: unmasked; otherwise every entry must be set) */
dvs_status dvs_orb_extract_batch_masked(dvs_orb* h, const uint8_t* const* imgs, int32_t nimg, int32_t rows, int32_t cols, size_t step,
                                        const uint8_t* const* masks, size_t mask_step, dvs_keypoint* kps, uint8_t* desc, int32_t capacity,
                                        int32_t* n_out);
/* frame f's mask at d_masks + f * mask_frame_stride; mask_frame_stride = 0: one mask for every frame (a static hood mask, say).
 * Read on the handle's stream by the filter behind FAST: keep it unchanged until the call's outputs are complete. */
dvs_status dvs_orb_extract_batch_device_masked(dvs_orb* h, const uint8_t* d_imgs, int32_t nimg, int32_t rows, int32_t cols, size_t step,
                                               size_t frame_stride, const uint8_t* d_masks, size_t mask_step, size_t mask_frame_stride,
                                               dvs_keypoint* d_kps, uint8_t* d_desc, int32_t capacity, int32_t* d_n_out);
/* ---- level-sharded extraction for SMALL batches on several GPUs (SURVEY.md §8e "Partitioning") --------------------------------
 * With fewer frames in flight than GPUs, frame sharding leaves GPUs idle; the stages after the pyramid are independent per
 * level (ORBextractor.cpp:787, 894, 1123), so every rank takes the same frames and a subset of the LEVELS: it rebuilds the
 * (cheap) level chain up to its highest level, runs FAST / quad-tree / blur / descriptors for its levels only and writes a
 * level-slotted block {int32 counts[nimg][nlevels]; dvs_keypoint[nimg][K]; uint8 desc[nimg][K][32]}, K = sum(quota_l + 4), in which
 * level l owns fixed slots.  One all-gather of the blocks (dvs_comm_all_gather) and dvs_orb_merge_levels_device then restore
 * the reference's level-major output on every rank — bit-identical to dvs_orb_extract_batch_device.  level_mask: bit l = this
 * rank owns level l (dvslam_amd.dist.level_shards balances them by pixel count). */
size_t dvs_orb_level_block_bytes(const dvs_orb* h, int32_t nimg);
dvs_status dvs_orb_extract_levels_device(dvs_orb* h, const uint8_t* d_imgs, int32_t nimg, int32_t rows, int32_t cols, size_t step,
                                         size_t frame_stride, uint32_t level_mask, uint8_t* d_block /* 16-byte aligned, level_block_bytes */);
/* d_blocks: [world][dvs_orb_level_block_bytes] as gathered; level_owner[nlevels] (host): the rank whose block holds level l */
dvs_status dvs_orb_merge_levels_device(dvs_orb* h, const uint8_t* d_blocks, int32_t world, const int32_t* level_owner, int32_t nimg,
                                       dvs_keypoint* d_kps, uint8_t* d_desc, int32_t capacity, int32_t* d_n_out);

/* the pyramid of the LAST extract call (mvImagePyramid is a public member, ORBextractor.hpp:84); blurred = 1: the blurred levels */
dvs_status dvs_orb_get_level(dvs_orb* h, int32_t frame, int32_t level, int32_t blurred, uint8_t* dst, int32_t cap_bytes);
/* ======================================= B2: Hamming matcher =================================== */

typedef struct dvs_matcher dvs_matcher;
dvs_status dvs_matcher_create(int32_t device, dvs_matcher** out);
/* the same on a caller-owned hipStream_t from the start (NULL = the legacy default stream): the handle then never creates a
 * stream of its own.  Every HIP stream is a hardware queue; idle ones are not free ("Streams and hardware queues") */
dvs_status dvs_matcher_create_on_stream(int32_t device, void* hip_stream, dvs_matcher** out);
void dvs_matcher_destroy(dvs_matcher* m);
dvs_status dvs_matcher_set_stream(dvs_matcher* m, void* hip_stream);
dvs_status dvs_matcher_synchronize(dvs_matcher* m);

/* BFMatcher(NORM_HAMMING).match(query, train): per query row the arg-min Hamming distance over train rows,
 * lowest train index on ties; train_idx = -1 and dist = INT32_MAX when nt == 0.  Rows are 32 bytes. Host pointers. */
dvs_status dvs_match_hamming(dvs_matcher* m, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt,
                             int32_t* train_idx, int32_t* dist);
/* npairs independent jobs, device-resident: job p uses rows [0, d_nq[p]) of d_q + p*q_stride_rows*32 against rows
 * [0, d_nt[p]) of d_t + p*t_stride_rows*32; outputs at d_idx/d_dist + p*q_stride_rows.  Asynchronous. */
dvs_status dvs_match_hamming_batch_device(dvs_matcher* m, const uint8_t* d_q, const int32_t* d_nq, int32_t q_stride_rows,
                                          const uint8_t* d_t, const int32_t* d_nt, int32_t t_stride_rows, int32_t npairs,
                                          int32_t* d_idx, int32_t* d_dist);
/* The frontend's pattern (frontend.cpp:1096: current frame against the previous one) over a device-resident run of frames:
 * frame p (rows [0, d_n[p]) of d_desc + p*stride_rows*32) is matched against frame p-1; frame 0 against the caller's
 * predecessor (d_prev_desc / d_prev_n: e.g. the last frame of the previous batch, wherever it lives — no copy), or against
 * nothing when both are NULL.  Outputs at d_idx/d_dist + p*stride_rows.  Asynchronous. */
dvs_status dvs_match_hamming_sequence_device(dvs_matcher* m, const uint8_t* d_desc, const int32_t* d_n, int32_t stride_rows,
                                             int32_t nframes, const uint8_t* d_prev_desc, const int32_t* d_prev_n, int32_t* d_idx,
                                             int32_t* d_dist);
/* backend.cpp:1068-1077 shape: every (query, train) pair with distance < max_dist, (query, train)-ordered int32
 * triplets (q, t, dist).  *n_pairs = total found (may exceed cap; only the first cap are written). Host pointers. */
dvs_status dvs_match_hamming_thresh(dvs_matcher* m, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt,
                                    int32_t max_dist, int32_t* pairs, int32_t cap, int32_t* n_pairs);
/* BFMatcher(NORM_HAMMING).knnMatch(query, train, matches, k): per query row the first min(k, nt) train rows in ascending
 * (distance, train index), at train_idx/dist + i*k; unused slots -1 / INT32_MAX.  k >= 1 (else DVS_ERR_ARG); k = 1 is
 * dvs_match_hamming.  Host pointers. */
dvs_status dvs_match_hamming_knn(dvs_matcher* m, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, int32_t k,
                                 int32_t* train_idx, int32_t* dist);
/* the same for npairs device-resident jobs (layout of dvs_match_hamming_batch_device); outputs at (p*q_stride_rows + i)*k.
 * Asynchronous. */
dvs_status dvs_match_hamming_knn_batch_device(dvs_matcher* m, const uint8_t* d_q, const int32_t* d_nq, int32_t q_stride_rows,
                                              const uint8_t* d_t, const int32_t* d_nt, int32_t t_stride_rows, int32_t npairs, int32_t k,
                                              int32_t* d_idx, int32_t* d_dist);
/* BFMatcher(NORM_HAMMING, crossCheck = true).match / knnMatch(k = 1): query i keeps j = argmin_j d(i, .) only if
 * i = argmin_i d(., j) (lowest index on ties on both sides); otherwise train_idx = -1, dist = INT32_MAX.  Host pointers. */
dvs_status dvs_match_hamming_cross(dvs_matcher* m, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt,
                                   int32_t* train_idx, int32_t* dist);
/* the same for npairs device-resident jobs (layout of dvs_match_hamming_batch_device).  Asynchronous. */
dvs_status dvs_match_hamming_cross_batch_device(dvs_matcher* m, const uint8_t* d_q, const int32_t* d_nq, int32_t q_stride_rows,
                                                const uint8_t* d_t, const int32_t* d_nt, int32_t t_stride_rows, int32_t npairs,
                                                int32_t* d_idx, int32_t* d_dist);
/* BFMatcher(NORM_HAMMING).radiusMatch(query, train, matches, max_distance): every pair with (float)dist <= max_distance
 * (inclusive; negative or NaN: none), per query in the order std::sort by distance gives the train-ordered list.  CSR result:
 * offsets[nq + 1] (always written), then (train, dist) int32 pairs.  *n_total = pairs found (may exceed cap; only the first
 * cap are written).  Host pointers. */
dvs_status dvs_match_hamming_radius(dvs_matcher* m, const uint8_t* q, int32_t nq, const uint8_t* t, int32_t nt, float max_distance,
                                    int64_t* offsets, int32_t* pairs, int64_t cap, int64_t* n_total);

/* ======================= E: the multi-GPU exchange step ========================== */
/* One process per GPU; frames (or, for small batches, pyramid levels) are sharded over the ranks and extraction needs no
 * communication.  The match job (t, t-1) at a shard boundary needs the previous rank's last-frame descriptors: ONE
 * ncclAllGather of fixed-size blocks per step, over RCCL/xGMI, on the caller's stream.  The reference has no counterpart
 * (single process per node; frontend.cpp:1096 keeps prev_descriptors_ in host memory).  RCCL is dlopen'ed at first use.
 *
 * Bring-up: rank 0 calls dvs_comm_get_unique_id and hands the 128 bytes to the other ranks out of band (MPI_Bcast, a TCP
 * store, a file); every rank then calls dvs_comm_create (collective, blocks until all ranks arrived). */
typedef struct dvs_comm dvs_comm;
#define DVS_COMM_ID_BYTES 128
dvs_status dvs_comm_get_unique_id(uint8_t* id /* [DVS_COMM_ID_BYTES] */);
dvs_status dvs_comm_create(int32_t device, int32_t rank, int32_t world, const uint8_t* id, dvs_comm** out);
/* Loopback group for one-GPU rehearsals and tests: out[0 .. world) = `world` logical ranks of THIS process on ONE device, no RCCL.
 * Each rank must be driven by its own host thread with its own streams; a collective call (dvs_exchange_boundary,
 * dvs_comm_all_gather) blocks on the host until every rank of the group has made the same call (30 s, then it fails on all ranks),
 * then pulls the peers' blocks with device-to-device copies behind their events.  Same results as the RCCL communicator. */
#define DVS_COMM_MAX_LOOPBACK 16
dvs_status dvs_comm_create_loopback(int32_t device, int32_t world, dvs_comm** out /* [world] */);
/* Host-transport communicator: the same exchange step for a host that moves the blocks itself (MPI_Allgather, sockets, a
 * torch.distributed group).  `all_gather(user, send, recv, bytes)` gathers `bytes` from every rank into recv[rank * bytes] on HOST memory
 * and returns 0 on success; it is called in place (send == recv + this rank's slot).  With such a communicator dvs_exchange_boundary /
 * dvs_comm_all_gather take and return HOST pointers, ignore `stream`, run synchronously and touch no device: the rank logic — buffer
 * rotation, this rank's slot, the predecessor with its wrap-around to the previous call — is the code the RCCL communicator runs.
 * Not accepted by dvs_pipeline_attach_comm (its blocks are device memory). */
typedef int (*dvs_host_all_gather_fn)(void* user, const void* send, void* recv, size_t bytes_per_rank);
dvs_status dvs_comm_create_host(int32_t rank, int32_t world, dvs_host_all_gather_fn all_gather, void* user, dvs_comm** out);
int32_t dvs_comm_is_host(const dvs_comm* c);
/* the next dvs_exchange_boundary starts a new sequence (rank 0: no predecessor).  Call with the streams of earlier calls drained. */
dvs_status dvs_comm_reset_sequence(dvs_comm* c);
void dvs_comm_destroy(dvs_comm* c);
int32_t dvs_comm_rank(const dvs_comm* c);
int32_t dvs_comm_world(const dvs_comm* c);
int32_t dvs_comm_rccl_version(void);  /* ncclGetVersion code, 0 if RCCL is unavailable */
/* bytes of one rank's boundary block {descriptors[cap x 32], int32 n, padding to 64 B} */
size_t dvs_boundary_block_bytes(int32_t cap);
/* The exchange step, called once per GLOBAL BATCH with this rank's LAST frame of the batch.  Packs {d_desc_last (cap rows of 32 B,
 * 16-byte aligned), *d_n_last} into this rank's slot of a gather buffer owned by the communicator (three buffers used in turn,
 * allocated once per capacity), all-gathers in place on `stream`, and returns device pointers to the predecessor of this rank's
 * FIRST frame of the same batch in the global frame order: rank r >= 1 gets rank r - 1's block of this call, rank 0 gets the last
 * rank's block of the PREVIOUS call (both NULL on the first call: the sequence starts there).  The pointers stay valid until the
 * call after next.  Asynchronous. */
dvs_status dvs_exchange_boundary(dvs_comm* c, void* stream, const uint8_t* d_desc_last, const int32_t* d_n_last, int32_t cap,
                                 const uint8_t** d_prev_desc, const int32_t** d_prev_n);
/* plain all-gather of bytes_per_rank bytes per rank (level-sharded extraction gathers its per-level blocks with it) */
dvs_status dvs_comm_all_gather(dvs_comm* c, void* stream, const void* d_send, void* d_recv, size_t bytes_per_rank);

/* ======================= the streaming step: extract batch i + match batch i - 1 ================= */
/* The reference's frame loop (frontend.cpp:1084-1123: gray -> (*orb_extractor_)(...) -> orb_matcher_->match(current, previous)) for a
 * host that holds its frames in device memory B at a time.  ONE call per step enqueues the whole software-pipelined schedule that
 * bench.py times and tests/test_gpu_pipeline.py checks frame by frame against the oracle:
 *   - the extraction of batch i on the extractor's streams (next batch's pyramid beside FAST, blur beside the quad-tree, the
 *     descriptor stage deferred beside the NEXT step's FAST);
 *   - the B match jobs of batch i - 1 (frame t against t - 1; frame 0 against the last frame of batch i - 2, or against the frame a
 *     communicator's boundary exchange returns) on the match stream, released behind batch i's FAST;
 *   - `nsets` (>= 3 when pipelined) output sets in rotation, the extraction of step i + nsets gated on the last reader of set i.
 * pipelined = 0: the plain schedule — every batch's match behind its own extraction on one stream (nsets >= 1).
 * Small batches (lanes >= 2; automatic for batch <= DVS_PIPELINE_LANE_BATCH): the machine is mostly idle within one step and the
 * step is the latency of its kernel chain, so `lanes` independent extractor / matcher pairs, one stream each, take the steps in turn
 * — step i runs serially on lane i % lanes (pyramid -> FAST -> quad-tree -> blur -> descriptors -> its own match, no internal
 * forks), up to `lanes` steps in flight, ordered only where data flows: the match of batch i waits for batch i - 1's descriptors
 * (another lane), the extraction of step i + nsets for the readers of set i.  Results are those of any other schedule, bit for bit.
 * The handle owns extractors, matchers, streams, events and the output sets; nothing is allocated per step.  Not thread-safe. */
typedef struct dvs_pipeline dvs_pipeline;
typedef struct dvs_pipeline_params {
  dvs_orb_params orb;   /* max_batch is ignored (= batch) */
  int32_t batch;        /* B frames per step, tight rows: frame f at d_imgs + f * rows * cols */
  int32_t rows, cols;
  int32_t nsets;        /* output sets in rotation; 0 = 4 (lane schedule: two per lane); lanes are reduced to a divisor of nsets */
  int32_t pipelined;    /* 1: the software pipeline described above; 0: serial match */
  int32_t lanes;        /* pipelined only.  0 = by batch size (DVS_PIPELINE_MAX_LANES up to DVS_PIPELINE_LANE_BATCH frames, else 1); 1 = the
                           two-stream software pipeline; 2..DVS_PIPELINE_MAX_LANES = lanes.  The fourth lane's stream has the highest dispatch
                           priority: streams of one priority share four hardware queues with the process's default stream */
  int32_t quadtree_async; /* two-stream pipeline only.  1: the four-stream form — quad-tree on the extractor's auxiliary stream beside the next
                           step's FAST (dvs_orb_set_async_quadtree), descriptor stage on the match stream (dvs_orb_set_tail_stream), blur on the
                           main stream ahead of FAST; -1: off; 0 = by batch size (on for DVS_PIPELINE_LANE_BATCH < batch <= DVS_PIPELINE_ASYNC_BATCH:
                           measured +21 % at 8 frames per step, +13 % at 16, +3.5 % at 24, a tie at 28..32, -4 % at 64: profiles/r04_batch_sweep.json) */
} dvs_pipeline_params;
#define DVS_PIPELINE_ASYNC_BATCH 24
#define DVS_PIPELINE_MAX_LANES 4     /* four hardware queues run at a time on this part: a fifth lane collapses all of them (EXPERIMENTS.md) */
#define DVS_PIPELINE_LANE_BATCH 6    /* lanes = 0: batches up to this size run on lanes (four lanes against the four-stream form: +16 % at 5 frames, +14 % at 6, a tie at 7, -5 % at 8) */
/* results of one step's batch (device pointers into the handle's output set; valid until step + nsets is enqueued) */
typedef struct dvs_pipeline_set {
  const dvs_keypoint* d_kps;  /* [B][capacity] */
  const uint8_t* d_desc;      /* [B][capacity][32] */
  const int32_t* d_n;         /* [B] */
  const int32_t* d_idx;       /* [B][capacity] trainIdx of frame f's keypoints in frame f - 1 */
  const int32_t* d_dist;      /* [B][capacity] */
  void* ev_extracted;         /* hipEvent_t: keypoints / descriptors / counts complete */
  void* ev_matched;           /* hipEvent_t: the batch's match jobs complete (recorded when they are enqueued: one step late if pipelined) */
  int32_t capacity;
} dvs_pipeline_set;
enum { DVS_PIPELINE_NO_MATCH = 1 };   /* step flags: extraction only (per-stage timing passes) */
dvs_status dvs_pipeline_create(const dvs_pipeline_params* params, int32_t device, dvs_pipeline** out);
void dvs_pipeline_destroy(dvs_pipeline* p);
/* frames sharded contiguously over ranks: frame 0 of a batch is matched against the frame dvs_exchange_boundary
 * returns (one all-gather per global batch on the match stream) instead of the previous batch's last frame.  NULL detaches. */
dvs_status dvs_pipeline_attach_comm(dvs_pipeline* p, dvs_comm* comm);
/* step i: d_imgs = this step's batch, d_next_imgs = the batch the NEXT step will pass (its pyramid is built ahead), NULL if unknown */
dvs_status dvs_pipeline_step(dvs_pipeline* p, const uint8_t* d_imgs, const uint8_t* d_next_imgs, int32_t flags);
/* the match of the last extracted batch (the pipelined schedule runs it one step late); no-op for the serial schedule */
dvs_status dvs_pipeline_flush(dvs_pipeline* p);
dvs_status dvs_pipeline_synchronize(dvs_pipeline* p);
/* synchronise and restart the sequence at step 0 (the next batch has no predecessor) */
dvs_status dvs_pipeline_reset(dvs_pipeline* p);
int64_t dvs_pipeline_steps(const dvs_pipeline* p);   /* steps enqueued since creation / reset */
dvs_status dvs_pipeline_get_set(const dvs_pipeline* p, int64_t step, dvs_pipeline_set* out);
/* which schedule the handle runs */
int32_t dvs_pipeline_quadtree_async(const dvs_pipeline* p);   /* 1: the four-stream form is in use */
int32_t dvs_pipeline_nsets(const dvs_pipeline* p);    /* output sets in rotation */
int32_t dvs_pipeline_lanes(const dvs_pipeline* p);    /* 0: serial schedule, 1: two-stream software pipeline, >= 2: lanes */
/* ---- measurement (bench.py's per-stage report and roofline; results are unaffected) ----
 * The extractor's scheduling hooks that this step is composed of (announced next batch, after-FAST event, deferred outputs, reuse guard,
 * quad-tree / tail streams, single-stream handles) are internal to the library since round 5; libdvslam_hip_test.so exports them for the
 * tests that pin them one by one (include/dvslam_hip_test.h). */
enum { DVS_STAGE_PYRAMID = 0, DVS_STAGE_FAST = 1, DVS_STAGE_OCTREE = 2, DVS_STAGE_BLUR = 3, DVS_STAGE_DESCRIBE = 4, DVS_STAGE_COUNT = 5 };
/* 1: every kernel of an extraction alone on the main stream (no overlap inside a step: what per-kernel durations are measured with);
 * 0: the shipped schedule.  Synchronises; refused for the lane schedule (its handles have one stream for good). */
dvs_status dvs_pipeline_set_serialized(dvs_pipeline* p, int32_t on);
/* per-stage GPU time (hipEvents around every stage of lane 0's extractor): switch, then accumulated milliseconds and launch-sequence
 * counts per stage since the last reset (synchronises) */
dvs_status dvs_pipeline_stage_timing(dvs_pipeline* p, int32_t on);
dvs_status dvs_pipeline_get_stage_times(dvs_pipeline* p, double* ms /* [DVS_STAGE_COUNT] */, int64_t* calls /* [DVS_STAGE_COUNT] */, int32_t reset);

/* ======================= glue either side of the path =============== */
/* A dvs_matcher handle is the context (stream + scratch).  Host pointers unless the name says _device. */

/* cv::cvtColor(bgr, gray, COLOR_BGR2GRAY) on 8UC3 (frontend.cpp:1084).  variant 0 = OpenCV 4.x 15-bit coefficients
 * (B*3735 + G*19235 + R*9798 + 16384) >> 15, variant 1 = the 14-bit ones of older releases. */
dvs_status dvs_bgr_to_gray(dvs_matcher* ctx, const uint8_t* bgr, int32_t rows, int32_t cols, size_t step, uint8_t* gray, size_t gray_step,
                           int32_t variant);
dvs_status dvs_bgr_to_gray_device(dvs_matcher* ctx, const uint8_t* d_bgr, int32_t nimg, int32_t rows, int32_t cols, size_t step,
                                  size_t frame_stride, uint8_t* d_gray, size_t gray_step, size_t gray_frame_stride, int32_t variant);
/* filterDepth / isValidDepth (frontend.cpp:457-527): keep keypoints (and descriptor rows) whose pixel (std::round of pt) has
 * depth_u16 * 0.001f in [min_depth, max_depth]; order preserved; out_index = original indices (may be NULL). */
dvs_status dvs_filter_depth(dvs_matcher* ctx, const dvs_keypoint* kps, const uint8_t* desc, int32_t n, const uint16_t* depth, int32_t rows,
                            int32_t cols, size_t step_bytes, float min_depth, float max_depth, dvs_keypoint* out_kps, uint8_t* out_desc,
                            int32_t* out_index, int32_t* n_out);
/* nframes frames resident in HBM: frame f uses rows [0, d_n[f]) of the [nframes][stride_rows] blocks dvs_orb_extract_batch_device
 * wrote and the depth image at d_depth + f * frame_stride_bytes.  Asynchronous. */
dvs_status dvs_filter_depth_batch_device(dvs_matcher* ctx, const dvs_keypoint* d_kps, const uint8_t* d_desc, const int32_t* d_n,
                                         int32_t stride_rows, int32_t nframes, const uint16_t* d_depth, int32_t rows, int32_t cols,
                                         size_t step_bytes, size_t frame_stride_bytes, float min_depth, float max_depth,
                                         dvs_keypoint* d_out_kps, uint8_t* d_out_desc, int32_t* d_out_index, int32_t* d_n_out);
/* frontend.cpp:1126-1132: matches with (float)distance < max_distance as (queryIdx, trainIdx, distance) int32 triplets */
dvs_status dvs_filter_matches(dvs_matcher* ctx, const int32_t* train_idx, const int32_t* dist, int32_t n, float max_distance,
                              int32_t* out_triplets, int32_t* n_out);
/* publishKeyframe (frontend.cpp:732-776): float back-projection with the depth image, keep 0.3 < Z < 3.0, world = R * p + t
 * (R row-major 3x3, double).  world_xyz[3 * n_out], out_index = keypoint indices (= the message's landmark_id).
 * A keypoint whose rounded position lies outside the depth image is dropped — here, in dvs_publish_keyframe* and in
 * dvs_filter_depth* alike (the reference reads the depth image unchecked at frontend.cpp:737). */
dvs_status dvs_backproject(dvs_matcher* ctx, const dvs_keypoint* kps, int32_t n, const uint16_t* depth, int32_t rows, int32_t cols,
                           size_t step_bytes, float fx, float fy, float cx, float cy, const double* R, const double* t, double* world_xyz,
                           int32_t* out_index, int32_t* n_out);
/* ---- Keyframe.msg on the wire (dynamic_visual_slam_interfaces/msg/{Keyframe,Landmark,Observation}.msg) ------------------------
 * The frontend publishes one Keyframe per keyframe on /frontend/keyframe (frontend.cpp:200, 699-790) and the backend consumes it;
 * rmw serialises it as little-endian CDR.  dvs_publish_keyframe* run publishKeyframe's loop (depth gate, back-projection,
 * landmark_id = keypoint index, float64 pixels, 32-byte descriptor) and write that CDR payload directly, so an adapter hands
 * the bytes to rclcpp::SerializedMessage / publish_serialized_message without touching 2000 keypoints on the host. */
typedef struct dvs_keyframe_header {
  int32_t stamp_sec;           /* header.stamp */
  uint32_t stamp_nanosec;
  const char* frame_id;        /* header.frame_id ("camera_link", frontend.cpp:727); <= 63 characters */
  uint64_t keyframe_id;        /* Keyframe.frame_id */
  double translation[3];       /* pose.translation x y z  (t_, optical frame) */
  double rotation_xyzw[4];     /* pose.rotation x y z w   (Eigen::Quaterniond(R_).normalized()) */
} dvs_keyframe_header;
/* payload bytes if all n keypoints pass the depth gate (the size of the buffer to provide) */
size_t dvs_keyframe_cdr_capacity(const char* header_frame_id, int32_t n);
/* device-resident inputs (extractor outputs, 16UC1 depth), payload into d_out; *d_out_size = bytes needed (> cap: nothing
 * written), *d_n_out = landmarks.  R (row-major 3x3), t: host.  Asynchronous on the context's stream. */
dvs_status dvs_publish_keyframe_device(dvs_matcher* ctx, const dvs_keyframe_header* hdr, const dvs_keypoint* d_kps, const uint8_t* d_desc,
                                       int32_t n, const uint16_t* d_depth, int32_t rows, int32_t cols, size_t step_bytes, float fx, float fy,
                                       float cx, float cy, const double* R, const double* t, uint8_t* d_out, size_t cap,
                                       uint64_t* d_out_size, int32_t* d_n_out);
/* host pointers in, payload in `out` */
dvs_status dvs_publish_keyframe(dvs_matcher* ctx, const dvs_keyframe_header* hdr, const dvs_keypoint* kps, const uint8_t* desc, int32_t n,
                                const uint16_t* depth, int32_t rows, int32_t cols, size_t step_bytes, float fx, float fy, float cx, float cy,
                                const double* R, const double* t, uint8_t* out, size_t cap, size_t* out_size, int32_t* n_landmarks);
/* the subscriber's side: a received payload as flat arrays (any output pointer may be NULL); hdr->frame_id points into
 * frame_id_buf.  Host code, no GPU.  DVS_ERR_CAPACITY (with the counts set) when an array holds fewer than cap_n entries. */
dvs_status dvs_keyframe_unpack_cdr(const uint8_t* buf, size_t len, dvs_keyframe_header* hdr, char* frame_id_buf, size_t frame_id_cap,
                                   uint64_t* landmark_ids, double* landmark_xyz, uint64_t* obs_landmark_ids, double* obs_pixels,
                                   uint8_t* obs_desc, int32_t cap_n, int32_t* n_landmarks, int32_t* n_observations);
/* ---- the frontend's robust-estimation stages, as batched-hypothesis kernels ---------------------------
 * Two forms.  dvs_find_fundamental_ransac / dvs_solve_pnp_ransac: the library's own minimal solvers (8-point, P3P) over a documented
 * deterministic sampler — NOT OpenCV's sample sequence or kernels (7-point, EPnP); they implement the same estimator (threshold, confidence, iteration cap, the
 * adaptive stopping rule RANSACUpdateNumIters, error measures) over a documented deterministic sampler (`seed`; csrc/ransac.hip),
 * and parity is stated as a tolerance on the inlier set and the pose.  Host pointers.
 *
 * cv::findFundamentalMat(pts1, pts2, mask, cv::FM_RANSAC, threshold = 2.0, confidence = 0.99) as frontend.cpp:635, 1146-1147
 * call it: pts n x 2 float, x2^T F x1 = 0; inlier_mask[n] = 1 where max of the two squared epipolar distances <= threshold^2
 * for the best model.  F9 (row-major, unit Frobenius norm) may be NULL.  n < 8: mask of zeros, *n_inliers = 0. */
dvs_status dvs_find_fundamental_ransac(dvs_matcher* ctx, const float* pts1, const float* pts2, int32_t n, double threshold, double confidence,
                                       int32_t max_iters /* OpenCV default 1000 */, uint64_t seed, double* F9, uint8_t* inlier_mask,
                                       int32_t* n_inliers);
/* nprob independent problems in ONE launch sequence (the replay's per-frame gates are pose-independent: tools/replay_tracking.py
 * runs them for all frames at once): problem b = correspondences [offsets[b], offsets[b + 1]) of the concatenated arrays, sampler
 * seed seeds[b]; outputs concatenated / indexed the same way.  Every problem gets exactly what the single call gives it. */
dvs_status dvs_find_fundamental_ransac_batch(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets /* nprob + 1, offsets[0] = 0 */, const float* pts1,
                                             const float* pts2, double threshold, double confidence, int32_t max_iters, const uint64_t* seeds,
                                             double* F9 /* nprob x 9 or NULL */, uint8_t* inlier_mask /* offsets[nprob] */, int32_t* n_inliers /* nprob or NULL */);
/* cv::findFundamentalMat(pts1, pts2, mask, cv::FM_RANSAC, threshold, confidence) (frontend.cpp:635, 1146-1147) the way OpenCV 4.x
 * itself runs it, restated from the published algorithm (calib3d fundam.cpp / ptsetreg.cpp; csrc/ransac.hip k_f7_hypotheses,
 * k_lmeds_select): the sample sequence — ONE cv::RNG seeded with (uint64)-1, index = next() % n, drawn again while it repeats, whole
 * samples drawn again while their last point is collinear with two earlier ones — and the 7-point solver (two null vectors,
 * cv::solveCubic, one model per real root, F(3,3) = 1), errors compared as floats.  From 15 correspondences on RANSAC
 * (RANSACPointSetRegistrator: strictly better inlier count wins, adaptive stopping rule, no refit; *iterations = loop iterations run);
 * from 8 to 14 LMedS, as OpenCV switches (LMeDSPointSetRegistrator: a fixed 300 iterations at confidence 0.99, smallest MEDIAN error
 * wins, inliers within sigma = 2.5 * 1.4826 * (1 + 5 / (n - 7)) * sqrt(median) >= 0.001; fewer than 7 of them: F9 all zero — OpenCV
 * returns an empty matrix — with the mask still written).  F9 row-major with F[8] = 1 (0 where OpenCV sets it so), may be NULL.
 * OpenCV's maxIters default is 1000.  n < 8 (the reference never calls there, frontend.cpp:627): DVS_ERR_UNSUPPORTED.  PARITY UNPINNED
 * like everything else (no OpenCV in this image).  What cannot agree even in principle: a tie between two models of ONE sample,
 * whose order follows the null-space basis (OpenCV: SVD); and LMedS below 14 points, where every model's median is the error of one
 * of its own sample points — rounding noise — so that WHICH of the 300 samples wins (and becomes the 7-point inlier set) is decided
 * by the rounding of the solver at hand. */
dvs_status dvs_find_fundamental_cv(dvs_matcher* ctx, const float* pts1, const float* pts2, int32_t n, double threshold, double confidence,
                                   int32_t max_iters, double* F9, uint8_t* inlier_mask, int32_t* n_inliers, int32_t* iterations);
dvs_status dvs_find_fundamental_cv_batch(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts1, const float* pts2, double threshold,
                                         double confidence, int32_t max_iters, double* F9, uint8_t* inlier_mask, int32_t* n_inliers, int32_t* iterations);
/* host only (works without a GPU): the sample sequence of the call above — iteration i drew idx[model_points i ..]; *found =
 * iterations that have a sample (cv::RNG((uint64)-1), uniform(0, n) = next() % n, repeats and collinear samples drawn again).
 * pts1 = pts2 = NULL: a callback WITHOUT checkSubset — the 5-point samples of dvs_solve_pnp_ransac_cv (model_points = 5). */
dvs_status dvs_cv_ransac_subsets(const float* pts1, const float* pts2, int32_t n, int32_t model_points, int32_t iterations, int32_t* idx, int32_t* found);
/* cv::solvePnPRansac(obj, img, K, noArray, rvec, tvec, false, iterations = 100, reproj_err = 4.0, confidence = 0.99, inliers)
 * (frontend.cpp:911-921; zero distortion): obj n x 3 float (camera frame of the previous image), img n x 2 float,
 * K4 = {fx, fy, cx, cy}.  P3P hypotheses, best by inlier count, Levenberg-Marquardt refinement on the inliers (the
 * SOLVEPNP_ITERATIVE step).  rvec3 = Rodrigues vector, tvec3: x_cam = R X + t.  inliers: ascending indices (capacity n, may be
 * NULL).  *success = 0 (and zeros) when no model found or n < 4. */
dvs_status dvs_solve_pnp_ransac(dvs_matcher* ctx, const float* pts3d, const float* pts2d, int32_t n, const double* K4, int32_t iterations,
                                double reproj_err, double confidence, uint64_t seed, double* rvec3, double* tvec3, int32_t* inliers,
                                int32_t* n_inliers, int32_t* success);
/* batch form: inliers concatenated like the points (problem b's ascending indices at inliers + offsets[b]); rvec3 / tvec3 nprob x 3 */
dvs_status dvs_solve_pnp_ransac_batch(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts3d, const float* pts2d, const double* K4,
                                      int32_t iterations, double reproj_err, double confidence, const uint64_t* seeds, double* rvec3, double* tvec3,
                                      int32_t* inliers /* offsets[nprob] or NULL */, int32_t* n_inliers /* nprob or NULL */, int32_t* success /* nprob */);

/* cv::solvePnPRansac(points3d, points2d, K, no distortion, rvec, tvec, false, iterations, reproj_err, confidence, inliers) AS OPENCV 4.x
 * RUNS IT with its default flags for the reference's call (frontend.cpp:911-921: 100, 4.0, 0.99) — csrc/pnp_cv.h: the 5-point samples of
 * ONE cv::RNG((uint64)-1), the EPnP minimal solver, projectPoints + squared error + threshold in float, the adaptive iteration count
 * (RANSACUpdateNumIters, 5 model points), then solvePnP(SOLVEPNP_ITERATIVE) on the inliers of the best model (planar / DLT initialisation
 * + CvLevMarq, 20 iterations, FLT_EPSILON).  inliers: the best model's inlier indices in index order (capacity n), as OpenCV returns them.
 * success = 0 with a model: the refit could not be initialised, rvec / tvec are the RANSAC stage's (OpenCV returns false there too).
 * Fewer than 6 points: success 0, nothing else written (the reference returns before the call, frontend.cpp:900).  PARITY UNPINNED:
 * restated from the published sources; every SVD is a Jacobi eigen-decomposition here (same models to rounding).  On an EXACTLY planar
 * point set EPnP's fourth control point coincides with the centroid and M^T M gains a trivial three-dimensional null space that its
 * N <= 3 approximations cannot leave — in OpenCV as here; dvs_solve_pnp_ransac (P3P) has no such case. */
dvs_status dvs_solve_pnp_ransac_cv(dvs_matcher* ctx, const float* pts3d, const float* pts2d, int32_t n, const double* K4, int32_t iterations,
                                   double reproj_err, double confidence, double* rvec3, double* tvec3, int32_t* inliers, int32_t* n_inliers,
                                   int32_t* success, int32_t* iterations_run);
dvs_status dvs_solve_pnp_ransac_cv_batch(dvs_matcher* ctx, int32_t nprob, const int32_t* offsets, const float* pts3d, const float* pts2d, const double* K4,
                                         int32_t iterations, double reproj_err, double confidence, double* rvec3, double* tvec3, int32_t* inliers,
                                         int32_t* n_inliers, int32_t* success, int32_t* iterations_run);

/* Harris corner measure as cv::ORB scores keypoints (ORB::HARRIS_SCORE, the mode test_dbow2_integration.cpp:19 runs with:
 * OpenCV features2d orb.cpp HarrisResponses — integer 3x3 gradients over a block_size^2 window, response = (ab - c^2 - k(a+b)^2)
 * / (4 block_size 255)^4 in float; cv::ORB uses block_size 7, k 0.04).  x, y: integer pixel positions in this image (one pyramid
 * layer).  Points closer than block_size/2 + 1 to the border get 0 (OpenCV reads outside the layer there). block_size <= 8. */
dvs_status dvs_harris_responses(dvs_matcher* ctx, const uint8_t* img, int32_t rows, int32_t cols, size_t step, const int32_t* x,
                                const int32_t* y, int32_t n, int32_t block_size, float k, float* response);
dvs_status dvs_harris_responses_device(dvs_matcher* ctx, const uint8_t* d_img, int32_t rows, int32_t cols, size_t step, const int32_t* d_x,
                                       const int32_t* d_y, int32_t n, int32_t block_size, float k, float* d_response);
/* associateObservation + reprojectPoint (backend.cpp:1064-1173) for all observations of one category against a snapshot of
 * that category's landmarks (arrays in the database's iteration order): best[i] = index of the candidate with Hamming
 * distance < max_descriptor_distance and the smallest reprojection error < max_reprojection_distance (first on ties), or -1.
 * obs_px: nobs x (u, v) float; lm_xyz: nlm x 3 float (cv::Point3f); R, t: keyframe pose as extractPoseFromTransform gives it. */
dvs_status dvs_associate(dvs_matcher* ctx, const uint8_t* obs_desc, const float* obs_px, int32_t nobs, const uint8_t* lm_desc,
                         const float* lm_xyz, int32_t nlm, const double* R, const double* t, double fx, double fy, double cx, double cy,
                         double max_descriptor_distance, double max_reprojection_distance, int32_t* best);

/* The same, plus every observation's candidate list: cand_lm[cand_offsets[i] .. cand_offsets[i + 1]) = the landmarks with Hamming
 * distance < max_descriptor_distance for observation i, in landmark order (cand_offsets: nobs + 1 entries; *n_cand = total; if
 * it exceeds cand_cap nothing is written to cand_lm and DVS_ERR_CAPACITY is returned with *n_cand set).  The reference applies
 * associations one by one and re-triangulates the landmark after each (backend.cpp:758-777): include/dvslam/association.hpp
 * uses the lists to re-evaluate exactly the observations whose candidates moved, in observation order. */
dvs_status dvs_associate_candidates(dvs_matcher* ctx, const uint8_t* obs_desc, const float* obs_px, int32_t nobs, const uint8_t* lm_desc,
                                    const float* lm_xyz, int32_t nlm, const double* R, const double* t, double fx, double fy, double cx,
                                    double cy, double max_descriptor_distance, double max_reprojection_distance, int32_t* best,
                                    int64_t* cand_offsets, int32_t* cand_lm, int64_t cand_cap, int64_t* n_cand);

/* LandmarkInfo::triangulate (backend.cpp:439-613) for nlm landmarks in one launch (csrc/triangulate.hip; INTEGRATION.md "Triangulation").
 * Landmark l's views are [view_offsets[l], view_offsets[l + 1]) of view_kf / view_px, in observation_ids order: keyframe index into R
 * (nkf x 9, row-major) / t (nkf x 3) and the float pixel.  view_kf < 0 skips the view, as the reference skips an id its find_if does not
 * find; skipped views do not count.  The pose convention is x_cam = R X + t (P = K [R | t], C = -R^T t): KeyframeInfo::R / t unchanged
 * reproduce the reference (whose reprojectPoint reads the same R, t the other way round); (R^T, -R^T t) is the consistent binding.
 * Steps and roundings are the reference's, with two documented departures: the SVD's gamma is sqrt(p * p + beta * beta), not hypot,
 * and the parallax gate's atan2 is the device's (1 ulp).  status[l] says why a landmark kept its position (lm_xyz_out = lm_xyz_in, bit
 * for bit, unless DVS_TRI_UPDATED); lm_xyz_out may alias lm_xyz_in.  view_kf >= nkf, view_offsets[0] < 0 or decreasing offsets:
 * DVS_ERR_ARG.  Host pointers. */
typedef enum { DVS_TRI_UPDATED = 0, DVS_TRI_FEW_VIEWS, DVS_TRI_LOW_PARALLAX, DVS_TRI_DEGENERATE, DVS_TRI_REPROJECTION, DVS_TRI_DEPTH } dvs_tri_status;
dvs_status dvs_triangulate_landmarks(dvs_matcher* ctx, int32_t nkf, const double* R, const double* t, double fx, double fy, double cx, double cy,
                                     int32_t nlm, const int64_t* view_offsets /* nlm + 1 */, const int32_t* view_kf, const float* view_px /* 2 per view */,
                                     const float* lm_xyz_in, float* lm_xyz_out, int32_t* status);
/* the same on device pointers, enqueued on the context's stream; it reads view_offsets[nlm] back first (one 8-byte copy) to size the
 * scratch of landmarks with more than eight views.  The argument checks of the host form run per landmark on the device: a landmark
 * whose offsets or keyframe indices are out of range keeps its position with status DVS_ERR_ARG. */
dvs_status dvs_triangulate_landmarks_device(dvs_matcher* ctx, int32_t nkf, const double* d_R, const double* d_t, double fx, double fy, double cx,
                                            double cy, int32_t nlm, const int64_t* d_view_offsets, const int32_t* d_view_kf, const float* d_view_px,
                                            const float* d_lm_xyz_in, float* d_lm_xyz_out, int32_t* d_status);

/* ======================================= B3: bundle adjustment ================================= */

typedef struct dvs_ba dvs_ba;

typedef struct dvs_ba_summary {
  int32_t termination;          /* 0 CONVERGENCE, 1 NO_CONVERGENCE, 2 FAILURE (ceres::TerminationType order) */
  int32_t num_successful_steps; /* OptimizationResult::iterations_completed (bundle_adjustment.hpp:862) */
  int32_t num_iterations;
  int32_t linear_solver;        /* who solved the normal equations: 1 = the device (dvs_ba_solve_device), 2 = the host (dvs_ba_solve), 3 = dvs_ba_solve_global */
  double initial_cost, final_cost;
} dvs_ba_summary;

dvs_status dvs_ba_create(int32_t device, dvs_ba** out);
void dvs_ba_destroy(dvs_ba* h);
dvs_status dvs_ba_set_stream(dvs_ba* h, void* hip_stream);
dvs_status dvs_ba_synchronize(dvs_ba* h);

/* Problem in the optimiser's parameterisation (bundle_adjustment.hpp:92-165): K poses = world->camera quaternion
 * (w,x,y,z) + translation, L landmarks, R observations (cam_idx, lm_idx, uv).  pose_fixed / lm_fixed: 1 = constant block
 * (bundle_adjustment.hpp:781-785, 795-797).  Intrinsics and sigma exactly as passed (no sanity checks: backend.cpp:180). */
dvs_status dvs_ba_set_problem(dvs_ba* h, int32_t K, const double* q_wxyz, const double* t, int32_t L, const double* X,
                              int32_t R, const int32_t* cam_idx, const int32_t* lm_idx, const double* uv,
                              const uint8_t* pose_fixed, const uint8_t* lm_fixed,
                              double fx, double fy, double cx, double cy, double sigma_pixels, double huber_delta);
/* one evaluation at the current parameters: robustified cost 0.5*sum(rho), and (each nullable) loss-corrected residuals
 * R x 2, local pose Jacobians R x 2 x 6 (rotation tangent first, then translation), landmark Jacobians R x 2 x 3,
 * gradient (6K + 3L, fixed blocks zero).  Host output pointers. */
dvs_status dvs_ba_evaluate(dvs_ba* h, double* cost, double* residuals, double* J_pose, double* J_lm, double* grad);
/* raw (un-robustified) functor outputs as ceres::CostFunction::Evaluate delivers them: residuals R x 2, jacobians
 * wrt q (R x 2 x 4), t (R x 2 x 3), X (R x 2 x 3), row-major; any may be NULL. */
dvs_status dvs_ba_evaluate_raw(dvs_ba* h, double* residuals, double* J_q, double* J_t, double* J_X);
/* Gauss-Newton blocks: H_pp K x 6 x 6, H_ll L x 3 x 3, W R x 6 x 3 (pose-landmark block per observation), g (6K + 3L) */
dvs_status dvs_ba_normal_equations(dvs_ba* h, double* H_pp, double* H_ll, double* W, double* g, double* cost);
/* `iters` back-to-back evaluations (residuals + Jacobians + loss + reductions) with nothing copied to the host; for
 * throughput measurement.  Asynchronous. */
dvs_status dvs_ba_evaluate_device(dvs_ba* h, int32_t iters);
/* Levenberg-Marquardt + Schur complement with the trust-region schedule of ceres::Solve as configured at
 * bundle_adjustment.hpp:839-847.  Parameters are updated in place; read them back with dvs_ba_get_parameters. */
dvs_status dvs_ba_solve(dvs_ba* h, int32_t max_iterations, double function_tolerance, double gradient_tolerance,
                        double parameter_tolerance, dvs_ba_summary* summary);
/* The same solve with the linear algebra on the device (Jacobi scaling, LM diagonal, Schur complement, Cholesky of the
 * reduced camera system, back-substitution, model cost change, candidate point): one 64-byte status record crosses PCIe per
 * trial step instead of the W blocks.  Same trust-region decisions, fixed-order reductions; sums are associated differently
 * from dvs_ba_solve, so costs agree to rounding (tests: 1e-9 relative), not bit for bit.  Sliding-window shapes only:
 * <= 64 cameras, 1..16 of them free (more, up to 63, once dvs_ba_set_device_window allows it on this handle), a landmark observed
 * at most once per camera; DVS_ERR_UNSUPPORTED otherwise. */
dvs_status dvs_ba_solve_device(dvs_ba* h, int32_t max_iterations, double function_tolerance, double gradient_tolerance,
                               double parameter_tolerance, dvs_ba_summary* summary);
/* largest number of free cameras dvs_ba_solve_device accepts on this handle: 1..63.  Default 16 (the in-LDS solver).
 * Above 16 the reduced camera system (up to 378 x 378) is factored by the tiled solver: block columns in global memory, one launch
 * per step on the handle's stream; dvs_ba_summary::linear_solver is 1 for both.  Windows of 1..16 free cameras run the in-LDS solver
 * whatever the setting.  K <= 64 and "a landmark at most once per camera" are unchanged; beyond the limit dvs_ba_solve_device returns
 * DVS_ERR_UNSUPPORTED as before.  Outside 1..63: DVS_ERR_ARG.  May be called before or after dvs_ba_set_problem; no GPU work. */
dvs_status dvs_ba_set_device_window(dvs_ba* h, int32_t max_free_cameras);
int32_t dvs_ba_get_device_window(const dvs_ba* h);
/* Trust-region log of the last dvs_ba_solve / dvs_ba_solve_device (what ceres::Solver::Summary::iterations holds): one row of
 * 6 doubles per iteration = {radius the step was computed with, kind, cost change, model cost change, relative decrease,
 * candidate cost}; kind 0 = invalid step, 1 = accepted, 2 = rejected, 3 / 4 = parameter / function tolerance reached.
 * *n_rows = rows available; at most cap_rows are written (rows may be NULL). */
dvs_status dvs_ba_get_trace(const dvs_ba* h, double* rows, int32_t cap_rows, int32_t* n_rows);
dvs_status dvs_ba_get_parameters(dvs_ba* h, double* q_wxyz, double* t, double* X);
/* ---- Global BA: every keyframe on the device, matrix-free Schur PCG -------------------------------------------------------------
 * dvs_ba_solve_global runs the trust-region loop of dvs_ba_solve_device (same decisions, same tolerances, same 6-column log, one
 * status record per trial step) around an INEXACT linear solve whose cost follows the number of observations: preconditioned
 * conjugate gradients on the reduced camera system S, which is never formed.  No limit on K; no L x K or n x n array anywhere.  It
 * takes every problem dvs_ba_set_problem takes that has at least one observation and one camera that is not fixed (DVS_ERR_ARG
 * otherwise), a landmark observed twice in one camera included (two ordinary terms).
 *
 * The linear solve of one trial step at radius rho.  With the Jacobi scaling s_j = 1 / (1 + sqrt(H_jj)) fixed at the first Jacobian,
 * D = clamp(diag(H scaled), 1e-6, 1e32), per active landmark l  Vinv_l = (Hll_l scaled + D_l / rho)^-1, and per observation e of
 * camera cam(e) and landmark l(e)  Ws_e = the scaled 6 x 3 block W_e, Y_e = Ws_e Vinv_l(e), for each free camera c (not fixed):
 *   (S p)_c = (Hpp_c scaled + D_c / rho) p_c - sum_{obs e of c} Ws_e Vinv_l(e) ( sum_{obs f of l(e), cam(f) free} Ws_f^T p_cam(f) )
 *   b_c     = g_c scaled - sum_{obs e of c} Y_e g_l(e) scaled
 * Fixed cameras and inactive landmarks (fixed, or observed by nobody) contribute nothing; a camera nobody observes is its damped
 * diagonal block.  The step is stored as solved (camera part not negated), the sign back-substitution and candidate read.
 *   Active set      every camera that is not fixed is active, whether or not anyone observes it (dvs_ba_solve_device also asks for
 *                   an observation); landmarks as there: not fixed and observed.  A free camera nobody observes has b_c = 0, so its
 *                   step is zero and it keeps its bytes, but as an active block its |x_c|^2 counts in the squared norm of the point
 *                   that the parameter-tolerance test reads — in dvs_ba_solve_device it does not.
 *   Preconditioner  M_c^-1, M_c = Hpp_c scaled + D_c / rho - sum_{e of c} Y_e Ws_e^T (the 6 x 6 diagonal blocks of S, Ceres'
 *                   SCHUR_JACOBI), inverted by Cholesky; the inverse of the block's diagonal alone if a pivot is not positive.
 *   Iteration       x_0 = 0, r_0 = b, z = M^-1 r, p = z;  alpha = r.z / p.Sp, x += alpha p, r -= alpha S p, z = M^-1 r,
 *                   beta = r.z new / r.z old, p = z + beta p.  Stops at the first k >= 1 with |r_k|_2 <= eta |b|_2 (r_k the
 *                   recurrence's residual) or at max_pcg_iterations (0: max(100, 12 nc), nc = free cameras).  |b|_2 = 0 (no free
 *                   camera is coupled to an active landmark with a gradient): x = 0 is the solution, the solve ends with zero
 *                   iterations and the trial step is valid — the landmarks still take their own steps -Vinv_l g_l.
 *   Breakdown       p.Sp <= 0 or not finite, with |b|_2 > 0, ends the solve: before the first iteration the trial step is invalid,
 *                   later the current x is the step.
 *   Determinism     the landmark-side sum runs over the landmark's observations in the order of the observation arrays grouped by
 *                   camera; the camera-side sum per chunk of <= 256 observations by a fixed tree, chunks in order; dot products by
 *                   fixed per-thread strides and a fixed tree.  No floating-point atomics: two identical solves return identical bytes.
 * The model cost change is computed from the actual step, so it is right for an inexact one.  Launches: three plain kernels per PCG
 * iteration that return at once after the stopping iteration; the host enqueues them in batches and reads one small record per
 * batch — no grid-wide barrier, no persistent kernel. */
typedef struct dvs_ba_global_params {
  int32_t max_iterations;       /* 50 */
  int32_t max_pcg_iterations;   /* 0 = max(100, 12 x free cameras) */
  double function_tolerance, gradient_tolerance, parameter_tolerance;   /* 1e-6, 1e-10, 1e-8 */
  double eta;                   /* 0.1; in (0, 1) */
} dvs_ba_global_params;
typedef struct dvs_ba_global_summary {
  dvs_ba_summary ba;            /* ba.linear_solver = 3 */
  int32_t pcg_iterations;       /* over all trial steps */
  int32_t reserved;
} dvs_ba_global_summary;
dvs_status dvs_ba_default_global_params(dvs_ba_global_params* params);
/* params NULL: the defaults.  eta outside (0, 1), a negative limit or tolerance: DVS_ERR_ARG. */
dvs_status dvs_ba_solve_global(dvs_ba* h, const dvs_ba_global_params* params, dvs_ba_global_summary* out);
/* beside dvs_ba_get_trace, one row per trial step of the last dvs_ba_solve_global: PCG iterations run and the recurrence's |r| / |b|
 * at the end (either array may be NULL) */
dvs_status dvs_ba_get_pcg_trace(const dvs_ba* h, int32_t* iterations, double* rel_residual, int32_t cap_rows, int32_t* n_rows);
/* CameraPose::fromRt / toRt (bundle_adjustment.hpp:138-165, 192-212): caller-convention (R row-major 3x3, t) <->
 * optimiser (q_wxyz, translation).  Host arithmetic used by the SlidingWindowBA adapter. */
dvs_status dvs_ba_pose_from_rt(const double* R, const double* t, double* q_wxyz, double* trans);
dvs_status dvs_ba_pose_to_rt(const double* q_wxyz, const double* trans, double* R, double* t);

/* ============================ cv::ORB-compatible extractor ============================
 * Replaces cv::ORB::create(...)->detectAndCompute(image, noArray(), keypoints, descriptors)
 * (/root/reference/dynamic_visual_slam/test/test_dbow2_integration.cpp:19,38; OpenCV 4.x features2d/src/orb.cpp): pyramid from
 * level 0 with INTER_LINEAR_EXACT, FAST-9/16 with non-max suppression over whole levels, runByImageBorder(edge), retainBest
 * (std::nth_element + std::partition semantics: ties with the last kept response are all kept, the order is libstdc++'s), HARRIS
 * responses (7 x 7, k = 0.04), intensity-centroid angle, rBRIEF on the 7 x 7 Gaussian-blurred level.  Keypoints come back in
 * cv::KeyPoint layout (pt in level-0 coordinates, size = 31 * scale, response = HARRIS value or FAST score, octave = level).
 * Built: firstLevel = 0, WTA_K = 2, patchSize = 31 (cv::ORB's defaults), edge_threshold >= 19; anything else DVS_ERR_UNSUPPORTED.
 * Because retainBest keeps ties, the count is data dependent: DVS_ERR_CAPACITY (with *n_out = rows needed) when capacity is
 * too small; an empty image returns DVS_OK with *n_out = 0 (detectAndCompute returns without detecting). */
typedef struct dvs_cvorb dvs_cvorb;
typedef struct dvs_cvorb_params {
  int32_t nfeatures;       /* 500 */
  float scale_factor;      /* 1.2f */
  int32_t nlevels;         /* 8 */
  int32_t edge_threshold;  /* 31 */
  int32_t first_level;     /* 0 */
  int32_t wta_k;           /* 2 */
  int32_t score_type;      /* 0 = cv::ORB::HARRIS_SCORE, 1 = FAST_SCORE */
  int32_t patch_size;      /* 31 */
  int32_t fast_threshold;  /* 20 */
} dvs_cvorb_params;
dvs_status dvs_cvorb_create(const dvs_cvorb_params* params, int32_t device, dvs_cvorb** out);
void dvs_cvorb_destroy(dvs_cvorb* h);
dvs_status dvs_cvorb_detect_and_compute(dvs_cvorb* h, const uint8_t* gray, int32_t rows, int32_t cols, size_t step_bytes, dvs_keypoint* kps,
                                        uint8_t* desc /* capacity x 32 */, int32_t capacity, int32_t* n_out);
/* parity introspection: level `level` of the last call's pyramid (blurred = 1: after the Gaussian), tight rows */
dvs_status dvs_cvorb_get_level(dvs_cvorb* h, int32_t level, int32_t blurred, uint8_t* dst, int32_t cap_bytes, int32_t* w, int32_t* hgt);

/* ============================ the tracking front end: one call per RGB-D frame ================================
 * Frontend::syncCallback (frontend.cpp:1068-1324) as ONE handle and ONE call per frame (csrc/tracker.hip; INTEGRATION.md "Tracking
 * front end"): gray -> extract -> filterDepth -> match against the previous frame -> distance < 50 -> fundamental-matrix gate ->
 * feature culling -> estimateCameraPose (3D points from the PREVIOUS depth image, PnP, inverse motion, isMotionOutlier, pose
 * products) -> isKeyframe -> Keyframe.msg CDR -> state update.  The image is copied up; the two depth images (current and previous)
 * are kept in pinned host memory and the kernels read the pixels under the keypoints from there; keypoints, descriptors, matches, point
 * lists and masks stay in HBM between the stages (with fm_mode = 1 the correspondences of a gate are read back for OpenCV's sampler).  The
 * handle owns one extractor, one matcher context (on the extractor's stream) and the members syncCallback keeps: R_, t_, prev_kps_,
 * prev_descriptors_, prev_frame_depth_, the last keyframe's features, frames_since_last_keyframe_, keyframe_id_.  Not thread-safe.
 * With the library's own estimators frame t (counted from create / reset) seeds the gate against the previous frame with
 * seed_base + 2t, PnP with seed_base + 2t + 1, the keyframe gate with seed_base + 2t + 1000003. */
typedef struct dvs_tracker dvs_tracker;
typedef struct dvs_tracker_params {
  int32_t rows, cols;                  /* every frame's size */
  double fx, fy, cx, cy;               /* rgb_fx_ .. rgb_cy_ */
  dvs_orb_params orb;                  /* frontend.cpp:206: 1000, 1.2, 8, 20, 7; max_batch is ignored */
  float min_depth, max_depth;          /* 0.3 / 3.0 (filterDepth, estimateCameraPose, publishKeyframe) */
  int32_t max_hamming;                 /* 50: matches with distance < this (frontend.cpp:1127, 618) */
  double fm_threshold, fm_confidence;  /* 2.0 px / 0.99 (frontend.cpp:1147, 636) */
  int32_t fm_max_iters;                /* 1000, OpenCV's default */
  int32_t cull_max_new;                /* MAX_NEW_FEATURES 200 (frontend.cpp:1205) */
  float cull_min_response;             /* MIN_RESPONSE 50.0 (frontend.cpp:1206) */
  int32_t pnp_iterations;              /* 100 (frontend.cpp:919-921) */
  double pnp_reproj_err, pnp_confidence; /* 4.0 / 0.99 */
  int32_t kf_min_matches;              /* a keyframe when fewer than 150 consistent matches with the last one (frontend.cpp:651) */
  int32_t kf_max_frames;               /* ... or frames_since_last_keyframe_ > 30 (frontend.cpp:655) */
  double max_translation, max_rotation; /* isMotionOutlier: 0.5 m / 0.2 rad (frontend.cpp:550-551) */
  int32_t fm_mode, pnp_mode;           /* 0: dvs_find_fundamental_ransac / dvs_solve_pnp_ransac with the seeds above; 1: the _cv forms */
  uint64_t seed_base;
  int32_t gray_variant;                /* dvs_bgr_to_gray's variant for 3-channel input */
  int32_t reserved;
} dvs_tracker_params;
enum {                                 /* dvs_track_result::kf_criterion (bits) */
  DVS_KF_FIRST_FRAME = 1,              /* frontend.cpp:1295 */
  DVS_KF_NO_REFERENCE = 2,             /* the first isKeyframe call: has_last_keyframe_ was false (frontend.cpp:603-606) */
  DVS_KF_FEW_MATCHES = 4,              /* tracking_criterion (frontend.cpp:651) */
  DVS_KF_MAX_FRAMES = 8                /* frames_since_last_keyframe_ > 30 (frontend.cpp:655) */
};
typedef struct dvs_track_result {
  int64_t frame_index;                 /* t, counted from create / reset */
  int64_t keyframe_id;                 /* Keyframe.frame_id of this frame's message, -1 if it is no keyframe */
  int32_t n_extracted, n_filtered;     /* extractor output, after filterDepth */
  int32_t n_matches, n_geometric;      /* distance-filtered, after the fundamental-matrix gate (= n_matches when it is skipped) */
  int32_t n_pnp_points, n_pnp_inliers; /* 3D-2D correspondences built, inliers of the PnP model */
  int32_t n_backend;                   /* culled feature set (what a keyframe carries) */
  int32_t n_kf_matches, n_kf_geometric; /* the same two counts against the last keyframe; -1 where isKeyframe did not get there */
  int32_t first_frame, tracking_reset, fm_skipped, pnp_skipped, pnp_failed, motion_outlier, pose_updated, is_keyframe, kf_criterion;
  int32_t cdr_landmarks;               /* landmarks in the payload */
  int32_t reserved;
  uint64_t cdr_bytes;                  /* payload size (what cdr_out must hold); 0 if no keyframe or cdr_out is NULL */
  double rvec[3], tvec[3];             /* this frame's PnP result (zeros when it did not run or failed) */
  double R[9], t[3];                   /* R_ (row-major) and t_ after this frame */
} dvs_track_result;
void dvs_tracker_default_params(dvs_tracker_params* p);   /* the reference's constants; rows / cols / intrinsics stay zero */
dvs_status dvs_tracker_create(const dvs_tracker_params* params, int32_t device, dvs_tracker** out);
void dvs_tracker_destroy(dvs_tracker* h);
/* back to the state after create: the next frame is a first frame, R_ = I, t_ = 0, keyframe_id_ = 0, t = 0.  Synchronises. */
dvs_status dvs_tracker_reset(dvs_tracker* h);
dvs_status dvs_tracker_set_stream(dvs_tracker* h, void* hip_stream);   /* extractor and matcher context move to it */
dvs_status dvs_tracker_synchronize(dvs_tracker* h);
/* One frame.  image: host, 8UC1 (channels 1) or BGR 8UC3 (channels 3), `step` bytes between rows; depth_u16: host 16UC1 in
 * millimetres, depth_step bytes between rows.  When the frame is a keyframe and cdr_out is not NULL the Keyframe.msg payload
 * (dvs_publish_keyframe_device's, header.frame_id "camera_link", header.stamp as given) is written there; if it needs more than
 * cdr_cap bytes the call returns DVS_ERR_CAPACITY with out->cdr_bytes set — the frame has been processed and the state updated.
 * Any other error leaves the frame half done: call dvs_tracker_reset before tracking on (dvs_tracker_get_backend_features gives 0 rows). */
dvs_status dvs_tracker_track(dvs_tracker* h, const uint8_t* image, int32_t channels, size_t step, const uint16_t* depth_u16, size_t depth_step,
                             int32_t stamp_sec, uint32_t stamp_nanosec, dvs_track_result* out, uint8_t* cdr_out, size_t cdr_cap);
/* the last frame's culled feature set in order (kps / desc / sel_index — indices into the depth-filtered set — each nullable, `cap`
 * rows); *n = rows available.  This read-back is the caller's choice, not part of the per-frame path. */
dvs_status dvs_tracker_get_backend_features(dvs_tracker* h, dvs_keypoint* kps, uint8_t* desc, int32_t* sel_index, int32_t cap, int32_t* n);

/* ============================ motion segmentation from depth: keep masks for the extractor ====================
 * Which pixels of the current depth image are moving, decided from two depth images, the relative pose between them and the intrinsics
 * (csrc/motion_seg.hip; INTEGRATION.md "Motion segmentation"): a point that now occupies space an earlier frame saw as free has moved.
 * The output is an 8-bit mask of the current frame, 255 = keep, 0 = moving, level-0 sized — exactly what dvs_orb_extract*_masked reads.
 * The reference has no counterpart (it filters YOLO boxes, backend.cpp:746-751).  tests/motion_ref.py restates the rule in numpy and the
 * GPU tests compare bit for bit.
 *
 * Inputs: D_ref, D_cur 16UC1 depth in millimetres (rows x cols); fx, fy, cx, cy; R[9] (row-major), t[3] with X_ref = R X_cur + t.
 * Stage 1, seeds.  Every current pixel (u, v) on its own, FP64 throughout, no contraction, every expression evaluated left to right as
 * written.  valid(d) := min_depth_mm < d && d <= max_depth_mm (integers).
 *   d = D_cur[v][u]; invalid: no verdict
 *   z = d * 0.001, x = (u - cx) * z / fx, y = (v - cy) * z / fy
 *   xr = R[0]*x + R[1]*y + R[2]*z + t[0], yr and zr likewise (rows 1 and 2); zr <= 0: no verdict
 *   ur = floor(fx * xr / zr + cx + 0.5), vr = floor(fy * yr / zr + cy + 0.5); a verdict needs 1 <= ur <= cols - 2 && 1 <= vr <= rows - 2,
 *   compared as doubles before the conversion to integers
 *   all nine D_ref values of the 3 x 3 window around (ur, vr) must be valid; m = their integer minimum   (n_valid counts who gets here)
 *   tau = tau0_m + tau2_per_m * zr * zr;  SEED iff zr < m * 0.001 - tau, strictly
 * i.e. the point lies nearer to the reference camera than anything that camera saw around that ray.  A point behind the reference surface
 * is occluded, not moving: no seed.
 * Stage 2, components.  Seeds are labelled by 8-connectivity: label[p] = the linear index y * cols + x of the component's smallest-index
 * pixel, -1 off the seeds (so the labelling does not depend on any scheduling); area[root] = its pixel count (integer adds).  A seed is
 * DYNAMIC iff its component has area >= min_area.
 * Stage 3, mask.  mask[p] = 0 iff a dynamic pixel lies in the (2r+1) x (2r+1) square around p, r = dilate_radius; pixels outside the image
 * count as not dynamic; every other pixel is 255.
 * Known limit: an object displaced by less than its own width between the two frames still covers most of the space it covered before,
 * and only its leading part is found (a third of its width: about 40 % of its pixels) — compare against a frame several frames back.
 * The default tolerances are a starting point: they were NEVER fitted to a sensor. */
typedef struct dvs_motion dvs_motion;
typedef struct dvs_motion_params {
  int32_t rows, cols;                       /* 1..4096 each */
  double fx, fy, cx, cy;                    /* finite, fx, fy > 0 */
  int32_t min_depth_mm, max_depth_mm;       /* 300 / 3000: the tracker's gates; 0 <= min < max <= 65535 */
  double tau0_m, tau2_per_m;                /* 0.03 / 0.005; finite, >= 0 */
  int32_t min_area;                         /* 200; >= 1 */
  int32_t dilate_radius;                    /* 8; 0..31 */
} dvs_motion_params;
typedef struct dvs_motion_stats {           /* all exact */
  int32_t n_valid;                          /* pixels that reached the depth compare */
  int32_t n_seed;
  int32_t n_components, n_components_kept;  /* all / those with area >= min_area */
  int32_t n_dynamic;                        /* seeds of kept components */
  int32_t n_masked;                         /* zeros in the mask */
} dvs_motion_stats;
void dvs_motion_default_params(dvs_motion_params* p);   /* the defaults above; rows / cols / intrinsics stay zero */
/* DVS_ERR_ARG for parameters outside the ranges above, before any device work; then DVS_ERR_NO_DEVICE without a gfx950 (no CPU fallback).
 * The handle works on HIP's legacy default stream until dvs_motion_set_stream. */
dvs_status dvs_motion_create(const dvs_motion_params* params, int32_t device, dvs_motion** out);
void dvs_motion_destroy(dvs_motion* h);
dvs_status dvs_motion_set_stream(dvs_motion* h, void* hip_stream);   /* synchronises the old stream first */
/* One mask.  d_ref / d_cur: device 16UC1 images, `*_step` bytes between rows (>= 2 cols, even); d_mask: device, mask_step >= cols.  R, t:
 * host, must be finite.  A fixed sequence of launches on the handle's stream, nothing read back: with stats == NULL the call does not
 * synchronise; otherwise it waits and fills *stats.  Nothing of an earlier call survives into the next.  Bad arguments: DVS_ERR_ARG
 * before any device work. */
dvs_status dvs_motion_segment_device(dvs_motion* h, const uint16_t* d_ref, size_t ref_step, const uint16_t* d_cur, size_t cur_step, const double* R9,
                                     const double* t3, uint8_t* d_mask, size_t mask_step, dvs_motion_stats* stats);
/* the same with host pointers; synchronises */
dvs_status dvs_motion_segment(dvs_motion* h, const uint16_t* ref, size_t ref_step, const uint16_t* cur, size_t cur_step, const double* R9,
                              const double* t3, uint8_t* mask, size_t mask_step, dvs_motion_stats* stats);
/* ---- the tracker's opt-in (csrc/tracker.hip): dynamic regions out of the keypoint budget without outside help ----
 * p != NULL switches it on: rows / cols / intrinsics of *p are replaced by the tracker's, lag in 1..16.  From then on every frame's depth
 * image is also copied into a device ring of lag + 1 slots with the pose R_, t_ after that frame, and BEFORE the extraction of frame t the
 * mask of frame t against frame t - min(lag, frames since the sequence began) is computed and the extraction goes through
 * dvs_orb_extract_batch_device_masked.  A sequence begins at a first frame and at a frame that reset the tracking; the frame that begins
 * one, the frame after a tracking reset, and any frame without a reference in the ring are extracted unmasked.  The current pose is
 * predicted by constant velocity, T(t-1) o (T(t-2)^-1 o T(t-1)) — just T(t-1) when frame t-1 did not update the pose or t-2 is not in the
 * sequence; R_, t_ are camera-to-world, so R = R_ref^T R_pred, t = R_ref^T (t_pred - t_ref).  dvs_tracker_reset empties the ring.
 * p == NULL switches it off (the default): the tracker then allocates and launches nothing it did not before.  Synchronises. */
dvs_status dvs_tracker_set_motion_mask(dvs_tracker* h, const dvs_motion_params* p /* NULL: off */, int32_t lag);
/* what the last frame's extraction used, so that a caller can recompute it: the mask (host, step >= cols; all 255 when none was used), the
 * relative pose it was made with, the reference's frame index (-1: none) and the statistics (zeros when none).  Any output may be NULL. */
dvs_status dvs_tracker_get_motion_mask(dvs_tracker* h, uint8_t* mask, size_t step, double* R9, double* t3, int64_t* ref_frame_index,
                                       dvs_motion_stats* stats);

/* ============================ the mapping backend: one call per keyframe, the map kept on the device ==========================
 * Backend::syncCallback (backend.cpp:709-832), the window selection of bundleAdjustmentCallback (:892-945), updateOptimizedResults
 * (:1356-1392) and pruneLandmarks (:1249-1322) as ONE handle (csrc/backend.hip; INTEGRATION.md "Mapping backend").  The landmark table
 * (id, class, position, descriptor, observation_count, last_seen), the observation table (all_observations_) and the keyframe poses
 * live in HBM and grow by doubling; the id counters, the keyframe list (frame_id, stamp, observation_ids) and the sequential walk of
 * the association loop stay on the host.  Categories are int32 class ids: 0 is "unlabeled", the adapters intern the strings.  The
 * caller serialises the calls on a handle (the reference's timer and mutex are not part of it).
 *
 * One stated deviation: the reference walks std::unordered_map<uint64_t, LandmarkInfo>, whose iteration order decides which of two
 * candidates with EXACTLY equal reprojection error wins (backend.cpp:1106, strict <).  The handle orders a class's landmarks by
 * ascending id, so the lowest id wins; results are equal wherever no two candidates tie exactly.
 * Unpinned: pruneLandmarks' age is read as (double)(now_ns - last_seen_ns) / 1e9 against a strict >, our reading of
 * rclcpp::Duration::seconds(); no test against rclcpp itself backs it. */
typedef struct dvs_backend dvs_backend;
#define DVS_BACKEND_MAX_FILTERED 16
typedef struct dvs_backend_params {
  double fx, fy, cx, cy;               /* fx_ .. cy_ */
  double max_descriptor_distance;      /* 50 (backend.cpp:1074) */
  double max_reprojection_distance;    /* 5 (:1106) */
  int32_t window;                      /* 5 (:895) */
  int32_t prune_min_observations;      /* 2 (:1251) */
  double prune_max_age_sec;            /* 20 (:1252) */
  int32_t n_filtered;                  /* filtered_objects_ as class ids (:749) */
  int32_t filtered_class_ids[DVS_BACKEND_MAX_FILTERED];
  int32_t initial_capacity;            /* rows every table starts with (4096); tables double when full */
} dvs_backend_params;
typedef struct dvs_detection {         /* yolo_msgs Detection: bbox centre and size in pixels, the class as an interned id (> 0) */
  double cx, cy, w, h;
  int32_t class_id;
  int32_t reserved;
} dvs_detection;
typedef struct dvs_backend_result {
  int32_t n_kept, n_filtered;          /* observations stored / dropped by the filtered classes (:749-751) */
  int32_t n_associated, n_created;     /* observations matched to an existing landmark / landmarks created (n_kept = sum) */
  int32_t n_moved;                     /* distinct landmarks whose position this keyframe's triangulation replaced (:772) */
  int32_t reserved;
  int64_t first_observation_id;        /* next_observation_id_ / next_global_landmark_id_ before the keyframe: the ids assigned are */
  int64_t first_landmark_id;           /* first .. first + n_kept - 1 and first .. first + n_created - 1 */
} dvs_backend_result;
typedef struct dvs_backend_count {
  int64_t n_keyframes, n_observations, n_landmarks, next_observation_id, next_landmark_id;
} dvs_backend_count;
void dvs_backend_default_params(dvs_backend_params* p);   /* the reference's constants; the intrinsics stay zero, no class is filtered */
dvs_status dvs_backend_create(const dvs_backend_params* params, int32_t device, dvs_backend** out);
void dvs_backend_destroy(dvs_backend* h);
dvs_status dvs_backend_reset(dvs_backend* h);             /* empty map, both id counters 0; the tables keep their size */
/* syncCallback without the ROS and marker parts.  hdr: stamp, Keyframe.frame_id (hdr->keyframe_id; a repeat is DVS_ERR_ARG) and pose;
 * n rows of landmark_xyz (3 doubles), obs_pixels (2 doubles) and obs_desc (32 bytes) in message order; detections in message order.
 * An error leaves the map as it was before the call only if it is DVS_ERR_ARG; after any other, reset the handle. */
dvs_status dvs_backend_add_keyframe(dvs_backend* h, const dvs_keyframe_header* hdr, int32_t n, const double* landmark_xyz, const double* obs_pixels,
                                    const uint8_t* obs_desc, const dvs_detection* detections, int32_t ndet, dvs_backend_result* result);
/* the same on the payload of dvs_publish_keyframe / dvs_tracker_track (through dvs_keyframe_unpack_cdr) */
dvs_status dvs_backend_add_keyframe_cdr(dvs_backend* h, const uint8_t* payload, size_t len, const dvs_detection* detections, int32_t ndet,
                                        dvs_backend_result* result);
dvs_status dvs_backend_counts(dvs_backend* h, dvs_backend_count* out);
/* The BA window as bundleAdjustmentCallback builds it: the last min(window, nkf) keyframes (frame_id, R 9 row-major, t 3), their
 * observations in all_observations_ order (pixel 2 floats, landmark id, class, frame_id, and obs_lm_index = the landmark's row in the
 * list that follows, -1 if the map does not hold it), and the distinct (landmark id, class) pairs in ascending id with their positions.
 * Count-then-capacity: the three counts are always set; DVS_ERR_CAPACITY, nothing written, when one exceeds its capacity. */
dvs_status dvs_backend_get_window(dvs_backend* h, int32_t cap_kf, int32_t cap_obs, int32_t cap_lm, uint64_t* kf_frame_id, double* kf_R, double* kf_t,
                                  int32_t* n_kf, float* obs_px, uint64_t* obs_lm_id, int32_t* obs_class, uint64_t* obs_frame_id, int32_t* obs_lm_index,
                                  int32_t* n_obs, uint64_t* lm_id, int32_t* lm_class, float* lm_xyz, int32_t* n_lm);
/* updateOptimizedResults: poses by frame_id (R 9 row-major, t 3 each; unknown ids are skipped), landmark positions by (id, class)
 * (3 doubles each, stored as float; a pair the map does not hold is skipped) */
dvs_status dvs_backend_apply_optimized(dvs_backend* h, int32_t nposes, const uint64_t* frame_ids, const double* R, const double* t, int32_t nlm,
                                       const uint64_t* lm_ids, const int32_t* lm_class, const double* lm_xyz);
/* pruneLandmarks at time `now` with its cascade: landmarks with observation_count < prune_min_observations whose age exceeds
 * prune_max_age_sec leave, with every observation in their lists or naming them; keyframes' observation_ids lose those ids */
dvs_status dvs_backend_prune(dvs_backend* h, int32_t now_sec, uint32_t now_nanosec, int32_t* removed_landmarks, int32_t* removed_observations);
/* Getters for tests and adapters (each output nullable, count-then-capacity as above).  Landmarks in ascending id; observation ids as
 * CSR (obs_offsets: *n + 1 entries).  last_seen / stamps in nanoseconds. */
dvs_status dvs_backend_get_landmarks(dvs_backend* h, int32_t cap, int64_t cap_obs_ids, uint64_t* id, int32_t* class_id, float* xyz, uint8_t* desc,
                                     int32_t* observation_count, int64_t* last_seen_ns, int64_t* obs_offsets, uint64_t* obs_ids, int32_t* n,
                                     int64_t* n_obs_ids);
dvs_status dvs_backend_get_observations(dvs_backend* h, int32_t cap, uint64_t* id, uint64_t* frame_id, float* px, uint8_t* desc, int32_t* class_id,
                                        uint64_t* landmark_id, int32_t* n);
dvs_status dvs_backend_get_keyframes(dvs_backend* h, int32_t cap, int64_t cap_obs_ids, uint64_t* frame_id, int64_t* stamp_ns, double* R, double* t,
                                     int64_t* obs_offsets, uint64_t* obs_ids, int32_t* n, int64_t* n_obs_ids);

/* ======================= place recognition: DBoW2 vocabulary transform and keyframe database ===================================
 * The other half of the reference's test/test_dbow2_integration.cpp (its README: "Loop Closure Ready: DBoW2 vocabulary integration";
 * CMakeLists.txt:124-128 links DBoW2): OrbVocabulary (TemplatedVocabulary<FORB::TDescriptor, FORB>) and OrbDatabase
 * (TemplatedDatabase) over 32-byte ORB descriptors, on the device (csrc/bow.hip; INTEGRATION.md "Place recognition").  PARITY UNPINNED:
 * DBoW2 is not available to this project; the semantics are restated from the published sources (tests/bow_ref.py is the sequential
 * restatement the kernels equal bit for bit), not proven against the library.
 *
 * Vocabulary: a tree, node 0 the root; every other node has a parent, a 32-byte descriptor, a double weight and an ordered child list;
 * the leaves are the words, numbered 0, 1, ... in node-id order.  A feature descends from the root: at every node the child with the
 * smallest Hamming distance wins, the FIRST such child on ties (DBoW2 compares with a strict <), until the winner is a leaf: that is
 * its word, the leaf's weight its weight.  Its feature-vector node is the winner at level L - levelsup (the root, 0, when that is
 * <= 0).  Deviation 1: where the descent ends at a leaf above that level DBoW2 leaves the node id uninitialised; here it is that leaf.
 * A frame's BowVector: features whose weight is not > 0 contribute nothing; TF_IDF / TF: v[word] += weight in feature order (a repeated
 * addition, ((w + w) + w) + ..., not count * w); IDF / BINARY: v[word] = weight; then every value is divided by the L1 norm, summed
 * sequentially in ascending word id, if that is > 0.  Its FeatureVector: node id -> ascending feature indices, as CSR.
 * Only scoring 0 (L1_NORM, DBoW2's and ORBvoc.txt's default) is built: any other is DVS_ERR_UNSUPPORTED.  The direct index
 * (use_di) is the "loop candidates" block below, a handle of its own (dvs_loop_db).  vocabulary.create()
 * (test_dbow2_integration.cpp:158) is dvs_voc_train below.
 * A vocabulary handle enqueues on the caller's hipStream_t (NULL: the legacy default stream), as dvs_matcher_create_on_stream; it
 * creates no stream.  A database borrows its vocabulary (stream and scratch): the vocabulary must outlive it, and the two are one
 * handle as far as threads are concerned. */
typedef struct dvs_bow_vocab dvs_bow_vocab;
typedef struct dvs_bow_db dvs_bow_db;
enum { DVS_BOW_L1_NORM = 0, DVS_BOW_L2_NORM = 1, DVS_BOW_CHI_SQUARE = 2, DVS_BOW_KL = 3, DVS_BOW_BHATTACHARYYA = 4, DVS_BOW_DOT_PRODUCT = 5 };
enum { DVS_BOW_TF_IDF = 0, DVS_BOW_TF = 1, DVS_BOW_IDF = 2, DVS_BOW_BINARY = 3 };
#define DVS_BOW_MAX_K 32
#define DVS_BOW_MAX_L 10
/* OrbVocabulary::loadFromTextFile (test_dbow2_integration.cpp:91), the text format of the ORB-SLAM flavour of DBoW2: first line
 * "k L scoring weighting", then one line "parent_id is_leaf d0 ... d31 weight" per node; the node on the n-th such line has id n and is
 * appended to its parent's child list.  k in 2..DVS_BOW_MAX_K, L in 1..DVS_BOW_MAX_L.  DVS_ERR_ARG: an unreadable file, a malformed
 * line, a parent id that is not smaller than the node's own, a node with more than k children, a node marked as a leaf that has
 * children or one not so marked that has none, a weight that is not finite.  Nodes with fewer than k children and leaves above depth L
 * are fine.  The file is parsed and checked before the device is touched. */
dvs_status dvs_bow_vocab_load_text(int32_t device, void* hip_stream, const char* path, dvs_bow_vocab** out);
/* the same from arrays: row j (of n_nodes >= 0) describes node j + 1 — parent id, leaf flag, 32 descriptor bytes, weight */
dvs_status dvs_bow_vocab_from_arrays(int32_t device, void* hip_stream, int32_t k, int32_t L, int32_t scoring, int32_t weighting, int32_t n_nodes,
                                     const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc, const double* weight, dvs_bow_vocab** out);
void dvs_bow_vocab_destroy(dvs_bow_vocab* voc);
/* OrbVocabulary::size / empty / getBranchingFactor ... (test_dbow2_integration.cpp:94): any output may be NULL; n_nodes without the root */
dvs_status dvs_bow_vocab_info(const dvs_bow_vocab* voc, int32_t* k, int32_t* L, int32_t* scoring, int32_t* weighting, int32_t* n_nodes,
                              int32_t* n_words);
dvs_status dvs_bow_vocab_synchronize(dvs_bow_vocab* voc);
/* OrbVocabulary::transform(features, bow_vector, feature_vector, levelsup) (test_dbow2_integration.cpp:161 and, inside the database,
 * :109, :117) for one frame of n host rows.  Outputs, each group nullable: word_ids / word_values (ascending word id; cap_words >= n
 * entries) and *n_words; the FeatureVector as CSR — fv_nodes (ascending node id), fv_offsets (cap_fv + 1 entries), fv_features
 * (cap_fv >= n entries) and *n_fv_nodes; feat_word / feat_node / feat_weight (n entries each): every feature's word, node and weight,
 * weight-0 features included.  A capacity below n is DVS_ERR_CAPACITY before anything runs. */
dvs_status dvs_bow_transform(dvs_bow_vocab* voc, const uint8_t* desc, int32_t n, int32_t levelsup, int32_t* word_ids, double* word_values,
                             int32_t cap_words, int32_t* n_words, int32_t* fv_nodes, int32_t* fv_offsets, int32_t* fv_features, int32_t cap_fv,
                             int32_t* n_fv_nodes, int32_t* feat_word, int32_t* feat_node, double* feat_weight);
/* nframes device-resident frames in the layout of dvs_match_hamming_batch_device: frame f uses rows [0, d_n[f]) of d_desc +
 * f*stride_rows*32 (16-byte aligned).  Outputs (each nullable) are [nframes][stride_rows] blocks — d_fv_offsets [nframes][stride_rows + 1] —
 * with the per-frame counts d_n_words[nframes], d_n_fv_nodes[nframes].  Asynchronous on the vocabulary's stream. */
dvs_status dvs_bow_transform_batch_device(dvs_bow_vocab* voc, const uint8_t* d_desc, const int32_t* d_n, int32_t stride_rows, int32_t nframes,
                                          int32_t levelsup, int32_t* d_word_ids, double* d_word_values, int32_t* d_n_words, int32_t* d_fv_nodes,
                                          int32_t* d_fv_offsets, int32_t* d_fv_features, int32_t* d_n_fv_nodes, int32_t* d_feat_word,
                                          int32_t* d_feat_node, double* d_feat_weight);
/* OrbDatabase(vocabulary) (test_dbow2_integration.cpp:103): entries kept on the device as a grow-only CSR of (word id, value) */
dvs_status dvs_bow_db_create(dvs_bow_vocab* voc, dvs_bow_db** out);
void dvs_bow_db_destroy(dvs_bow_db* db);
dvs_status dvs_bow_db_clear(dvs_bow_db* db);          /* TemplatedDatabase::clear: no entries, the next id is 0 */
int32_t dvs_bow_db_size(const dvs_bow_db* db);        /* TemplatedDatabase::size (:113); 0 for NULL */
/* database.add(features) (:109): the frame's normalised BowVector becomes entry *entry_id = size() */
dvs_status dvs_bow_db_add(dvs_bow_db* db, const uint8_t* desc, int32_t n, int32_t* entry_id);
/* nframes device-resident frames (layout of dvs_bow_transform_batch_device) become entries *first_entry_id_out + f.  Asynchronous. */
dvs_status dvs_bow_db_add_device(dvs_bow_db* db, const uint8_t* d_desc, const int32_t* d_n, int32_t stride_rows, int32_t nframes,
                                 int32_t* first_entry_id_out);
/* database.query(features, results, max_results, max_id) (:117) with L1 scoring: for every entry e (e < max_id unless max_id == -1) that
 * shares a word with the query's vector q, raw = sum over the common words, in ascending word id, of |q_i - e_i| - |q_i| - |e_i|;
 * entries without a common word do not appear.  Deviation 2: the results are ordered by ascending (raw, entry id) — the lowest id wins
 * among equal raws, as everywhere in this library — where DBoW2 runs an unstable std::sort on raw alone; the two agree wherever no two
 * raws tie exactly.  The first max_results (all if max_results <= 0) are written as ids / scores with score = -raw / 2.0; *n_results =
 * their number.  cap below min(max_results or all, admissible entries) is DVS_ERR_CAPACITY before anything runs. */
dvs_status dvs_bow_db_query(dvs_bow_db* db, const uint8_t* desc, int32_t n, int32_t max_results, int32_t max_id, int32_t* ids, double* scores,
                            int32_t cap, int32_t* n_results);
/* the same on device pointers: rows [0, *d_n) of d_desc (16-byte aligned, stride_rows rows allocated), results and count to device
 * memory.  Asynchronous. */
dvs_status dvs_bow_db_query_device(dvs_bow_db* db, const uint8_t* d_desc, const int32_t* d_n, int32_t stride_rows, int32_t max_results,
                                   int32_t max_id, int32_t* d_ids, double* d_scores, int32_t cap, int32_t* d_n_results);
/* read-back of entry `id` for tests and adapters: *n = its words (always set); DVS_ERR_CAPACITY, nothing written, if cap < *n */
dvs_status dvs_bow_db_get_entry(dvs_bow_db* db, int32_t id, int32_t* word_ids, double* word_values, int32_t cap, int32_t* n);

/* ----------------------- vocabulary training: OrbVocabulary::create (test_dbow2_integration.cpp:138-163) --------------------------
 * DBoW2's TemplatedVocabulary::create, HKmeansStep, initiateClustersKMpp, FORB::meanValue and setNodeWeights, restated from the
 * published sources (PARITY UNPINNED, as above; tests/bow_train_ref.py is the recursive restatement csrc/bow_train.hip equals bit for
 * bit).  The training set is nimages images, each an ordered list of 32-byte descriptors; `features` is all of them in image order.
 *   create   the root is node 0; step(root, all features, level 1); the words are the leaves in ascending node id; then the weights.
 *   step(parent, F, level)   nothing if F is empty.  |F| <= k: one cluster per feature in order (centre i = F[i], group i = {i}).
 *     Otherwise k-means++ seeds, then passes: (1) from the second pass on every centre becomes the mean of its group, (2) every
 *     feature joins the centre of smallest Hamming distance, the FIRST such centre on ties (strict <), (3) from the second pass on
 *     stop when no association changed.  Groups keep their members in ascending position within F.  One node per cluster is appended
 *     in cluster order (consecutive ids, descriptor = centre, parent = `parent`); then, if level < L, step(child i, group i, level + 1)
 *     for i = 0, 1, ... where group i has more than one member.  So a node's children have contiguous ids and everything below child 0
 *     precedes everything below child 1; a node above depth L whose group has at most one member is a leaf.
 *   mean   bit b of the mean of N >= 1 descriptors is set iff at least N/2 + N%2 of them have it set.
 *   seeding   the first centre is the feature at a drawn position; min_dist[i] = distance to the closest centre so far; while fewer
 *     than k centres: S = sum(min_dist) (exact, 64 bits); S == 0 stops (fewer than k children: duplicate features); else with a drawn
 *     cut in 1..S the next centre is the feature at the first position whose inclusive prefix sum of min_dist is >= cut.
 *   sampler   DBoW2 seeds DUtils::Random from the clock, so there is nothing to reproduce; here every node has a key —
 *     key(root) = splitmix64(seed), key(child c of a node with key K) = splitmix64(K ^ (c + 1)), c 0-based — and draw j of the node is
 *     u_j = splitmix64(K + j * 0x9E3779B97F4A7C15): the first position is u_0 mod |F|, the j-th further centre uses cut = 1 + u_j mod S.
 *     It does not depend on the order in which nodes are processed.
 *   deviation 3 (iteration cap)   DBoW2's loop has none and could cycle; here a node runs at most max_iterations association passes
 *     and keeps the centres and groups of its last pass (report: nodes_capped).
 *   deviation 4 (emptied cluster)   DBoW2 would take the mean of an empty set; here the cluster keeps its previous centre and ends as a
 *     childless node no training feature reaches: Ni = 0, weight 0 (report: clusters_emptied, counted over the final groups).
 *   weights   TF / BINARY: 1.0 per word.  TF_IDF / IDF: every training feature is transformed with the finished tree; Ni[w] = images
 *     with at least one feature on word w; weight = log((double)nimages / (double)Ni[w]) where Ni > 0, else 0.0, computed on the host
 *     (glibc's log) from device-counted integers; inner nodes weigh 0.0.  ONE training image therefore gives all-zero weights (size() > 0,
 *     every BowVector empty): that is DBoW2's behaviour.
 * report: levels_run = the deepest level that got nodes; max_passes = the most association passes any node ran; nodes_short_seeded =
 * nodes whose seeding stopped at S == 0.  The result is an ordinary dvs_bow_vocab bound to (device, hip_stream).
 * DVS_ERR_ARG before any device work: k outside 2..DVS_BOW_MAX_K, L outside 1..DVS_BOW_MAX_L, a negative count, max_iterations < 1, a NULL
 * array with a non-zero count, a weighting outside 0..3; DVS_ERR_UNSUPPORTED: a scoring other than L1_NORM.  No features at all: an empty
 * vocabulary and DVS_OK.  The call runs on the caller's stream, creates none, and SYNCHRONISES that stream: convergence is read back
 * (one word per few passes) and the tree's new nodes once per level.  No floating point on the device. */
typedef struct { int32_t k, L, weighting, scoring; uint64_t seed; int32_t max_iterations; } dvs_voc_train_params;
typedef struct { int32_t n_nodes, n_words, levels_run, max_passes, nodes_capped, clusters_emptied, nodes_short_seeded; } dvs_voc_train_report;
/* k 10, L 5, TF_IDF, L1_NORM (DBoW2's constructor defaults), seed 0, max_iterations 100 */
dvs_status dvs_voc_train_default_params(dvs_voc_train_params* params);
/* host rows: desc = all images' rows concatenated, image_counts[nimages]; report may be NULL */
dvs_status dvs_voc_train(int32_t device, void* hip_stream, const dvs_voc_train_params* params, const uint8_t* desc, const int32_t* image_counts,
                         int32_t nimages, dvs_bow_vocab** out, dvs_voc_train_report* report);
/* device-resident frames in the layout of dvs_bow_transform_batch_device (counts clamped to 0..stride_rows, at most 65535 frames): the
 * extractor's or the tracker's blocks train it in place */
dvs_status dvs_voc_train_device(int32_t device, void* hip_stream, const dvs_voc_train_params* params, const uint8_t* d_desc, const int32_t* d_n,
                                int32_t stride_rows, int32_t nframes, dvs_bow_vocab** out, dvs_voc_train_report* report);
/* any vocabulary back as dvs_bow_vocab_from_arrays takes it: *n_nodes always set; DVS_ERR_CAPACITY, nothing written, if cap < *n_nodes;
 * each array may be NULL.  Synchronises the vocabulary's stream. */
dvs_status dvs_voc_get_arrays(const dvs_bow_vocab* voc, int32_t cap, int32_t* parent, uint8_t* is_leaf, uint8_t* desc, double* weight,
                              int32_t* n_nodes);
/* TemplatedVocabulary::saveToTextFile in the format dvs_bow_vocab_load_text reads; weights with 17 significant digits (they round-trip) */
dvs_status dvs_voc_save_text(const dvs_bow_vocab* voc, const char* path);

/* ----------------------- loop candidates: a keyframe database with a direct index, and node-guided matching ----------------------
 * What a loop detector does between database.query() and its robust estimators (dvs_find_fundamental_*, dvs_solve_pnp_ransac_*):
 * correspondences between the new keyframe and each candidate, compared only inside the vocabulary node two features share
 * (csrc/loop.hip; INTEGRATION.md "Loop candidates").  Neither DBoW2's direct index nor any loop detector is a reference interface this
 * project can pin: the FeatureVector an entry keeps is DBoW2's (retrieveFeatures), the MATCHING RULE below is this library's own,
 * stated in full and independent of any processing order, as the sampler of dvs_voc_train is.  Integers only: results are bit-exact
 * (tests/loop_ref.py is the sequential restatement).
 *
 * Direct index.  A database is created over a vocabulary with di_levels >= 0.  add runs ONE transform of the frame at levelsup =
 * di_levels; the BowVector does not depend on levelsup, so the stored entry and every query result are those of dvs_bow_db_add / query
 * (the same kernels).  The entry also keeps its FeatureVector (node id -> ascending feature indices, exactly what dvs_bow_transform
 * returns: features whose word weight is not > 0 are absent, deviation 1 applies, di_levels >= L puts every feature under node 0) and
 * all n descriptor rows of the frame, so feature indices stay frame indices.  Everything stays on the device.
 *
 * Guided match of a query frame Q (n rows) against entry e with (max_distance, ratio_num, ratio_den): for every node present in both
 * FeatureVectors (both at levelsup = di_levels) and every query feature i under it, over the entry's features j under the same node in
 * ascending j: d1 = the smallest Hamming distance, j1 = the lowest j that attains it, d2 = the smallest distance among j != j1 (256
 * when the node holds one entry feature).  i PROPOSES (j1, d1) iff d1 <= max_distance and d1 * ratio_den <= d2 * ratio_num.  Among the
 * query features that propose the same j the one with the smallest (d1, i) keeps it, the others are unmatched.  (An entry feature lies
 * under exactly one node, so conflicts never cross nodes.)  Output per candidate c and row i < stride_rows: train_idx = j or -1,
 * dist = d1 or INT32_MAX; rows i >= n are written as unmatched; n_matches[c] = the candidate's count.  An entry id outside [0, size)
 * gives n_matches[c] = -1 and all rows unmatched in the device forms, DVS_ERR_ARG before any device work in the host form.  The same
 * id may appear twice in a candidate list: each occurrence gets the same answer.
 * Parameters, not constants: the defaults are max_distance 50 and ratio 3/4, the values guided ORB matchers usually run with (quoted
 * from memory, not pinned to any library).  DVS_ERR_ARG: max_distance outside 0..256, ratio_den outside 1..32767, ratio_num outside
 * 0..32767.  A NULL params pointer means the defaults.  One call matches at most 65535 candidates (n_cand, cap_cand, or the most
 * results detect's query can give: more is DVS_ERR_ARG), and candidates x max(rows of the frame, rows of the longest entry) must stay
 * below 2^31.
 *
 * The handle borrows its vocabulary's stream and scratch as dvs_bow_db does: the vocabulary must outlive it, and the two are one handle
 * as far as threads are concerned.  NULL handles are DVS_ERR_ARG, capacity checks come before any device work, and there is no CPU
 * fallback (a vocabulary cannot be created without a device: DVS_ERR_NO_DEVICE). */
typedef struct dvs_loop_db dvs_loop_db;
typedef struct { int32_t max_distance, ratio_num, ratio_den; } dvs_loop_match_params;
dvs_status dvs_loop_match_default_params(dvs_loop_match_params* p);   /* 50, 3, 4 */
/* TemplatedDatabase(voc, use_di = true, di_levels) */
dvs_status dvs_loop_db_create(dvs_bow_vocab* voc, int32_t di_levels, dvs_loop_db** out);
void dvs_loop_db_destroy(dvs_loop_db* db);
dvs_status dvs_loop_db_clear(dvs_loop_db* db);            /* no entries, the next id is 0; the blocks keep their size */
int32_t dvs_loop_db_size(const dvs_loop_db* db);          /* 0 for NULL */
int32_t dvs_loop_db_di_levels(const dvs_loop_db* db);     /* getDirectIndexLevels; -1 for NULL */
/* database.add(features): entry *entry_id = size() with its BowVector, FeatureVector and rows.  Synchronises. */
dvs_status dvs_loop_db_add(dvs_loop_db* db, const uint8_t* desc, int32_t n, int32_t* entry_id);
/* nframes device-resident frames in the layout of dvs_bow_transform_batch_device become entries *first_entry_id + f.  The host does
 * not know d_n: it reserves stride_rows rows per frame (the true counts are read back before a block grows).  Asynchronous. */
dvs_status dvs_loop_db_add_device(dvs_loop_db* db, const uint8_t* d_desc, const int32_t* d_n, int32_t stride_rows, int32_t nframes,
                                  int32_t* first_entry_id);
/* dvs_bow_db_query / dvs_bow_db_query_device: the same arguments, the same results, the same kernels */
dvs_status dvs_loop_db_query(dvs_loop_db* db, const uint8_t* desc, int32_t n, int32_t max_results, int32_t max_id, int32_t* ids, double* scores,
                             int32_t cap, int32_t* n_results);
dvs_status dvs_loop_db_query_device(dvs_loop_db* db, const uint8_t* d_desc, const int32_t* d_n, int32_t stride_rows, int32_t max_results,
                                    int32_t max_id, int32_t* d_ids, double* d_scores, int32_t cap, int32_t* d_n_results);
/* TemplatedDatabase::retrieveFeatures(id) as CSR: fv_nodes (ascending; cap_nodes entries), fv_offsets (cap_nodes + 1 entries),
 * fv_features (cap_features entries), each nullable.  Count-then-capacity: *n_nodes and *n_features are always set; DVS_ERR_CAPACITY,
 * nothing written, if one exceeds its capacity. */
dvs_status dvs_loop_db_get_features(dvs_loop_db* db, int32_t id, int32_t* fv_nodes, int32_t* fv_offsets, int32_t* fv_features, int32_t cap_nodes,
                                    int32_t cap_features, int32_t* n_nodes, int32_t* n_features);
/* read-back of entry `id`'s rows for tests and adapters: *n always set; DVS_ERR_CAPACITY, nothing written, if cap_rows < *n */
dvs_status dvs_loop_db_get_descriptors(dvs_loop_db* db, int32_t id, uint8_t* desc, int32_t cap_rows, int32_t* n);
/* guided match of one host frame against n_cand entries (host ids): train_idx / dist are [n_cand][n], n_matches [n_cand].  Synchronises. */
dvs_status dvs_loop_db_match(dvs_loop_db* db, const uint8_t* desc, int32_t n, const int32_t* entry_ids, int32_t n_cand,
                             const dvs_loop_match_params* params, int32_t* train_idx, int32_t* dist, int32_t* n_matches);
/* the same with everything on the device: rows [0, *d_n) of d_desc (16-byte aligned, stride_rows rows allocated), candidates
 * d_entry_ids[0, *d_n_cand) with *d_n_cand clamped to 0..cap_cand — the ids / count dvs_loop_db_query_device wrote feed it with nothing
 * crossing to the host.  Outputs d_train_idx / d_dist [cap_cand][stride_rows], d_n_matches [cap_cand]; blocks c >= *d_n_cand are
 * written as unmatched with n_matches 0.  Asynchronous. */
dvs_status dvs_loop_db_match_device(dvs_loop_db* db, const uint8_t* d_desc, const int32_t* d_n, int32_t stride_rows, const int32_t* d_entry_ids,
                                    const int32_t* d_n_cand, int32_t cap_cand, const dvs_loop_match_params* params, int32_t* d_train_idx,
                                    int32_t* d_dist, int32_t* d_n_matches);
/* ONE transform of the frame, the query (max_results, max_id as in dvs_loop_db_query: max_id excludes recent keyframes), then the guided
 * match of the results, all in one enqueue; one read-back returns ids / scores / n_matches [*n_results] and train_idx / dist
 * [*n_results][n] (arrays of cap and cap * n entries; cap below the most results the query can give is DVS_ERR_CAPACITY). */
dvs_status dvs_loop_db_detect(dvs_loop_db* db, const uint8_t* desc, int32_t n, int32_t max_results, int32_t max_id,
                              const dvs_loop_match_params* params, int32_t* ids, double* scores, int32_t* n_matches, int32_t* train_idx,
                              int32_t* dist, int32_t cap, int32_t* n_results);
/* the same on device pointers: d_ids / d_scores / d_n_matches [cap], d_train_idx / d_dist [cap][stride_rows], *d_n_results.  Asynchronous. */
dvs_status dvs_loop_db_detect_device(dvs_loop_db* db, const uint8_t* d_desc, const int32_t* d_n, int32_t stride_rows, int32_t max_results,
                                     int32_t max_id, const dvs_loop_match_params* params, int32_t* d_ids, double* d_scores, int32_t* d_n_matches,
                                     int32_t* d_train_idx, int32_t* d_dist, int32_t cap, int32_t* d_n_results);

/* ----------------------- loop verification: rigid 3D-3D RANSAC over the candidates of one detect, on the device -------------------
 * The step after the guided match: for every candidate the rigid motion between the two keyframes' cameras, estimated from the metric
 * 3D points both keyframes of an RGB-D system carry (csrc/loop_verify.hip; INTEGRATION.md "Loop candidates").  It reads train_idx where
 * match / detect left it on the device and returns one small record per candidate.  No loop detector is a reference interface this
 * project can pin, so the RULE is the library's own, stated here in full and restated sequentially in tests/loop_verify_ref.py: integer
 * parts (gathered lists, samples, counts, selection, masks) are exact, float parts are FP64 on the float inputs and carry tolerances
 * (tests/test_gpu_loop_verify.py states them).
 *
 * Points.  The direct index holds one more per-row block: xyz, three floats per descriptor row, in the entry keyframe's camera frame.
 * add / add_device store no points: rows never given points hold NaN.  dvs_loopv_db_set_points* fill an entry's rows, dvs_loop_db_clear
 * forgets them.  A point is VALID iff its three coordinates are finite and z > 0; a keypoint without depth is any invalid point.
 *
 * Model: x_q = R x_e + t, from the entry's camera frame to the query's, scale 1 (Sim(3) is out of scope).
 * Per candidate c < clamp(*d_n_cand, 0, cap_cand), entry e = d_entry_ids[c]:
 *  1 gather    the correspondence list: every query row i < clamp(*d_n, 0, stride_rows), in ascending i, with j = train_idx[c][i] in
 *              [0, rows of e), query point i and entry point j both valid.  m entries; n_corr = m.  e outside [0, size): n_corr = -1
 *              and the candidate fails.  m < min_correspondences: the candidate FAILS (success 0, n_inliers 0, iterations 0, pose and
 *              rms zeros, mask zeros).
 *  2 hypotheses  seed_c = splitmix64(seed ^ (uint64)e), so the answer does not depend on the candidate's position in the list.
 *              Hypothesis h < iterations draws 3 distinct list positions with the sampler of dvs_solve_pnp_ransac (draw j of
 *              hypothesis h is the r-th position not drawn before, r = splitmix64(seed_c + 0x9E3779B97F4A7C15 * (16 h + j + 1)) mod
 *              (m - j)) and fits Horn's closed form (Horn 1987, "Closed-form solution of absolute orientation using unit
 *              quaternions"): the centroids, the 3 x 3 cross-covariance S = sum (x_e - mean_e)(x_q - mean_q)^T of the centred triples,
 *              the symmetric 4 x 4 matrix N of S, its eigenvector of the largest eigenvalue (cyclic Jacobi), sign q0 >= 0, R from
 *              the unit quaternion, t = mean_q - R mean_e.  A hypothesis is DEGENERATE, with count 0, if anything is not finite or
 *              (lambda1 - lambda2) <= 1e-9 |lambda1| for the two largest eigenvalues (collinear or coincident samples).
 *  3 score     the error of correspondence k under (R, t) is the larger of two squared reprojection distances, with K4 = {fx, fy,
 *              cx, cy}: in the query image between the projections of R x_e + t and x_q, in the entry image between the projections
 *              of R^T (x_q - t) and x_e; +inf if either transformed depth is <= 0.  k is an inlier iff error <= reproj_err^2.
 *  4 select    the sequential RANSAC loop replayed over the counts, as in dvs_solve_pnp_ransac: hypothesis h is iteration h, a count
 *              above max(best, 2) becomes the best and shortens the loop by cv::RANSACUpdateNumIters(confidence, (m - count) / m, 3,
 *              iterations).  `iterations` of the record = iterations run.  No hypothesis with more than 2 inliers: the candidate fails.
 *  5 refine    S_0 = the inliers of the selected hypothesis.  For r = 1 .. refine_rounds: Horn on S_(r-1) (centroids first, then
 *              the centred covariance; partial sums folded in a fixed order, no floating atomics: two identical calls give identical
 *              bytes), S_r = the inliers of that fit; accepted iff the fit is not degenerate and |S_r| >= |S_(r-1)|, else the rounds
 *              stop and round r-1's model and set stay.
 *  6 result    n_inliers = |S|, rvec = the principal Rodrigues vector of R (the conversion dvs_solve_pnp_ransac ends in), tvec = t,
 *              rms_px = sqrt(mean inlier error), success = n_inliers >= min_inliers (the pose, count and mask are reported either way);
 *              inlier_mask[c][i] (uint8, query rows) = 1 exactly for the inlier correspondences' i, 0 for every other i < stride_rows.
 * Slots c >= *d_n_cand are written as failed with n_corr 0.  The same id may appear twice: each occurrence gets the same record.
 * Parameters, not constants: the defaults are 256 iterations, min_correspondences 12, min_inliers 12, refine_rounds 2, reproj_err 4.0
 * px (the value the reference passes to solvePnPRansac, frontend.cpp:911-921), confidence 0.99, seed 0 — usual values, not pinned to
 * any library; K4 has no default, so a NULL params pointer is DVS_ERR_ARG (dvs_loopv_default_params leaves K4 zeros: zeros are
 * refused).  DVS_ERR_ARG: iterations outside 1..4096, min_correspondences < 3, min_inliers < 3, refine_rounds outside 0..8, reproj_err
 * or a focal length not > 0, confidence outside (0, 1), anything not finite.  The limits of the match apply (65535 candidates,
 * candidates x rows below 2^31) and candidates x iterations must stay below 2^31.  Scratch belongs to the handle and grows on demand;
 * capacity checks come before any device work.
 * Names: the functions carry the prefix dvs_loopv_ ("loop verification"), not dvs_loop_: tests/test_loop_cpu.py pins the exact set of
 * dvs_loop_* symbols the library exports, and existing tests stay as they are.  They take the same dvs_loop_db handle. */
typedef struct {
  int32_t iterations, min_correspondences, min_inliers, refine_rounds;
  double reproj_err, confidence;
  uint64_t seed;
  double K4[4];
} dvs_loop_verify_params;
typedef struct {
  int32_t n_corr, n_inliers, success, iterations;
  double rvec[3], tvec[3], rms_px;
} dvs_loop_verify_result;
dvs_status dvs_loopv_default_params(dvs_loop_verify_params* p);   /* 256, 12, 12, 2, 4.0, 0.99, 0, K4 zeros (to be set) */
/* entry entry_id's points from the host: n must equal the entry's row count (DVS_ERR_ARG otherwise, and for an id outside [0, size)).
 * Synchronises. */
dvs_status dvs_loopv_db_set_points(dvs_loop_db* db, int32_t entry_id, const float* xyz, int32_t n);
/* the points of entries first_entry_id + f, f < nframes, in the layout of dvs_loop_db_add_device: frame f's rows start at d_xyz + 3 * f *
 * stride_rows; one kernel copies min(clamp(d_n[f], 0, stride_rows), rows of the entry) rows per entry.  Asynchronous. */
dvs_status dvs_loopv_db_set_points_device(dvs_loop_db* db, int32_t first_entry_id, const float* d_xyz, const int32_t* d_n, int32_t stride_rows,
                                         int32_t nframes);
/* read-back of entry `id`'s points (NaN where none were set): *n always set; DVS_ERR_CAPACITY, nothing written, if cap_rows < *n */
dvs_status dvs_loopv_db_get_points(dvs_loop_db* db, int32_t id, float* xyz, int32_t cap_rows, int32_t* n);
/* the verification on exactly the buffers dvs_loop_db_detect_device / match_device wrote: d_xyz_query [stride_rows][3], d_train_idx
 * [cap_cand][stride_rows]; outputs d_results [cap_cand], d_inlier_mask [cap_cand][stride_rows].  Nothing crosses to the host.
 * Asynchronous. */
dvs_status dvs_loopv_db_verify_device(dvs_loop_db* db, const float* d_xyz_query, const int32_t* d_n, int32_t stride_rows, const int32_t* d_entry_ids,
                                     const int32_t* d_n_cand, int32_t cap_cand, const int32_t* d_train_idx, const dvs_loop_verify_params* params,
                                     dvs_loop_verify_result* d_results, uint8_t* d_inlier_mask);
/* host form: xyz [n][3], train_idx and inlier_mask [n_cand][n], results [n_cand]; an entry id outside [0, size) is DVS_ERR_ARG before any
 * device work.  Synchronises. */
dvs_status dvs_loopv_db_verify(dvs_loop_db* db, const float* xyz, int32_t n, const int32_t* entry_ids, int32_t n_cand, const int32_t* train_idx,
                              const dvs_loop_verify_params* params, dvs_loop_verify_result* results, uint8_t* inlier_mask);
/* dvs_loop_db_detect followed by the verification of its results: transform, query, guided match and verification in ONE enqueue with
 * ONE read-back.  Outputs as dvs_loop_db_detect's plus results [cap] and inlier_mask [cap][n]. */
dvs_status dvs_loopv_db_detect_verify(dvs_loop_db* db, const uint8_t* desc, const float* xyz, int32_t n, int32_t max_results, int32_t max_id,
                                     const dvs_loop_match_params* match_params, const dvs_loop_verify_params* verify_params, int32_t* ids,
                                     double* scores, int32_t* n_matches, int32_t* train_idx, int32_t* dist, dvs_loop_verify_result* results,
                                     uint8_t* inlier_mask, int32_t cap, int32_t* n_results);

/* ======================================= Pose-graph optimisation ================================= */
/* The consumer of a verified loop (csrc/pose_graph.hip): a sparse SE(3) least-squares solve over ALL keyframes, and the correction that
 * moves the landmarks along with their keyframes.  The rule is the library's own (PARITY UNPINNED: stated here in full, restated
 * sequentially in float64 in tests/pose_graph_ref.py; no g2o, GTSAM or Ceres is compared against).  FP64 throughout.
 *  Nodes     N poses (R_i, t_i) with x_world = R_i x_i + t_i, given as R (9 doubles, row-major) and t — the layout dvs_backend_get_keyframes
 *            returns, in the direction dvs_associate's reprojection reads it (x_cam = R^T (X - t)) — and a `fixed` flag per node.  The handle keeps the poses as given ("before") and the current ones.  The current
 *            rotation is kept as a unit quaternion (w, x, y, z), made from R by Shepperd's rule (the largest of w, x, y, z first) and
 *            normalised; dvs_pgo_get_nodes returns the R made from it (1 - 2(yy + zz), 2(xy - wz), ...), also before any solve.
 *  Edges     E records (i, j, rvec, tvec, w_rot, w_trans).  The measurement Z = (R_z, t_z), R_z = cos(a) I + (1 - cos(a)) k k^T + sin(a) [k]x
 *            for rvec = a k (the identity for the zero vector), means x_i = R_z x_j + t_z, that is Z ~ T_i^-1 T_j.  A verified loop is
 *            the edge (query, entry, result.rvec, result.tvec) unchanged; odometry between consecutive keyframes has the same form.
 *            Duplicate edges are allowed (each counts).
 *  Residual  6 per edge: r = [ w_rot Log(R_z^T R_i^T R_j) ; w_trans R_z^T (R_i^T (t_j - t_i) - t_z) ], with Log(Q): v = vee(Q - Q^T) / 2,
 *            s = |v|, c = (tr Q - 1) / 2, theta = atan2(s, c), omega = v theta / s if s > 1e-12, else v.  Rotation errors beyond about
 *            3.1 rad are OUTSIDE THE DOMAIN (v vanishes at pi and the axis is lost).  Cost = 0.5 sum |r|^2.  There is no robust loss: the
 *            RANSAC gate of the verification is the defence against false loops.
 *  Update    delta_i = (omega, v): R_i <- R_i Exp(omega), t_i <- t_i + R_i v, both with the R_i before the step.  Jacobians are the exact
 *            derivatives of r in delta_i, delta_j at delta = 0, two 6 x 6 blocks per edge (row = residual, column = delta), with
 *            M = R_i^T R_j, Q = R_z^T M, p = R_i^T (t_j - t_i), Jr^-1 = I + [omega]x / 2 + c [omega]x^2, c = 1 / theta^2 - (1 + cos theta) /
 *            (2 theta sin theta) (theta < 1e-2: 1/12 + theta^2 / 720 + theta^4 / 30240):
 *              Ji = [ -w_rot Jr^-1 M^T, 0 ; w_trans R_z^T [p]x, -w_trans R_z^T ]      Jj = [ w_rot Jr^-1, 0 ; 0, w_trans Q ].
 *            The block of a fixed node is zero, and its rows are not part of the linear system (gradient rows exactly 0).  The quaternion
 *            is updated as q <- q * (cos(|omega| / 2), sin(|omega| / 2) omega / |omega|) and renormalised at every step.
 *  Outer loop  Levenberg-Marquardt under the trust-region policy of dvs_ba_solve (csrc/ba.hip, struct TrustRegion, restated in
 *            pose_graph.hip): initial radius 1e4; accepted when cost_change / model_cost_change > 1e-3; radius /= max(1/3, 1 - (2 rho - 1)^3)
 *            on success (at most 1e16), /= 2, 4, 8 .. on failure; the LM diagonal D = clamp(diag(H), 1e-6, 1e32) (0 on fixed nodes) is kept
 *            across a rejected step and rebuilt after any other; five invalid steps in a row (a step that is not finite, or a model
 *            change that is not > 0) fail the solve.  model_cost_change = -(x.g + 0.5 |J x|^2).  Tolerances as there: max |g_k| over the
 *            free coordinates <= gradient_tolerance at the loop head; |candidate - current| <= parameter_tolerance (|current| +
 *            parameter_tolerance) over (q, t) of the free nodes, and |cost_change| <= function_tolerance cost, both on the candidate
 *            before acceptance.  No Jacobi column scaling.
 *  Linear solve  (H + D / radius) x = -g with H = J^T J never assembled: preconditioned conjugate gradients from x = 0; the preconditioner is
 *            the inverse of the 6 x 6 diagonal blocks of H + D / radius (Cholesky; the inverse of its diagonal if a pivot is not positive).
 *            It stops at the first iteration k >= 0 with |r_k|_2 <= eta |g|_2 (r_k the recurrence's residual) or at max_pcg_iterations
 *            (0: max(100, 2 N)).  An isolated free node has a zero gradient and does not move.
 *  Determinism  every sum folds in a fixed order — per node over its incident edges in ascending edge index, dot products as per-thread
 *            strided partial sums folded by a fixed tree — and there are no floating-point atomics: two identical solves return
 *            identical bytes.
 * DVS_ERR_ARG, before any device work (dvs_pgo_check_graph makes the same checks without a handle or a device): no fixed node; i == j; an
 * index outside [0, N); a weight not > 0; anything not finite; N outside 1..2^20 or E outside 1..2^22; edges set before nodes.  Setting
 * nodes of another count drops the edges; setting the same count again keeps them (a second solve from the same start).
 * Every N and E in range runs: a linear solve is ONE workgroup striding over nodes and edges, with its vectors in global memory.
 * One small status record per trial step crosses to the host, as in dvs_ba_solve_device; nothing else does.  Calls on one handle are
 * serial; the handle owns its stream. */
typedef struct dvs_pgo dvs_pgo;
typedef struct dvs_pgo_params {
  int32_t max_iterations, max_pcg_iterations;     /* 50; 0 = max(100, 2 N) */
  double function_tolerance, gradient_tolerance, parameter_tolerance;   /* 1e-6, 1e-10, 1e-8 */
  double eta;                                     /* 0.1; in (0, 1) */
} dvs_pgo_params;
typedef struct dvs_pgo_summary {
  int32_t termination;          /* 0 converged, 1 iteration limit, 2 failure */
  int32_t num_successful_steps, num_iterations;
  int32_t pcg_iterations;       /* over all trial steps */
  double initial_cost, final_cost;
} dvs_pgo_summary;
dvs_status dvs_pgo_default_params(dvs_pgo_params* p);
/* the argument checks of dvs_pgo_set_nodes and dvs_pgo_set_edges on their own: host code, no handle, no device */
dvs_status dvs_pgo_check_graph(int32_t N, const double* R, const double* t, const uint8_t* fixed, int32_t E, const int32_t* i, const int32_t* j,
                               const double* rvec, const double* tvec, const double* w_rot, const double* w_trans);
dvs_status dvs_pgo_create(int32_t device, dvs_pgo** out);
void dvs_pgo_destroy(dvs_pgo* h);
dvs_status dvs_pgo_synchronize(dvs_pgo* h);
/* R [N][9], t [N][3], fixed [N]: "before" and current both become these poses */
dvs_status dvs_pgo_set_nodes(dvs_pgo* h, int32_t N, const double* R, const double* t, const uint8_t* fixed);
/* i, j [E], rvec, tvec [E][3], w_rot, w_trans [E]; builds the node -> edge lists once */
dvs_status dvs_pgo_set_edges(dvs_pgo* h, int32_t E, const int32_t* i, const int32_t* j, const double* rvec, const double* tvec, const double* w_rot,
                             const double* w_trans);
/* at the current poses: cost, residuals [E][6], Ji, Jj [E][36] (row-major), grad [6 N]; every output nullable.  The counterpart of
 * dvs_ba_evaluate. */
dvs_status dvs_pgo_evaluate(dvs_pgo* h, double* cost, double* residuals, double* Ji, double* Jj, double* grad);
/* from the current poses; params NULL: the defaults.  Synchronises. */
dvs_status dvs_pgo_solve(dvs_pgo* h, const dvs_pgo_params* params, dvs_pgo_summary* summary);
dvs_status dvs_pgo_get_nodes(dvs_pgo* h, double* R, double* t);   /* the current poses; either may be NULL */
/* as dvs_ba_get_trace, one row of 7 doubles per trial step: radius, kind (0 invalid, 1 accepted, 2 rejected, 3 parameter tolerance, 4
 * function tolerance), cost_change, model_cost_change, rho, candidate cost, PCG iterations of the step */
dvs_status dvs_pgo_get_trace(const dvs_pgo* h, double* rows, int32_t cap_rows, int32_t* n_rows);
/* Map correction: for a = anchor[k] in [0, N): x' = R'_a (R_a^T (x - t_a)) + t'_a, unprimed "before", primed current — computed in FP64 in
 * exactly that operation order (sums left to right) and rounded to float once, from the same R bytes dvs_pgo_get_nodes returns.  Any other
 * anchor leaves the point untouched.  In place on xyz [n][3].  The host form synchronises; the device form is asynchronous on the
 * handle's stream (dvs_pgo_synchronize). */
dvs_status dvs_pgo_correct_points(dvs_pgo* h, int32_t n, float* xyz, const int32_t* anchor);
dvs_status dvs_pgo_correct_points_device(dvs_pgo* h, int32_t n, float* d_xyz, const int32_t* d_anchor);

/* ======================================= Loop closing on the map ================================= */
/* Verified loops applied to the map the mapping backend keeps on the device (csrc/loop_close.hip; INTEGRATION.md "Loop closure"): the
 * step ORB-SLAM calls CorrectLoop (Mur-Artal, Montiel, Tardos 2015, section VII-C: pose-graph optimisation, then every map point moved
 * with a keyframe that observes it) and the one it calls SearchAndFuse (duplicated map points merged), both as published ideas.  The
 * reference has no loop closing, so there is no reference interface to pin: PARITY UNPINNED, the rule is the library's own, stated
 * here in full and restated sequentially in tests/loop_closing_ref.py.
 *  Anchors   The anchor of a landmark is the keyframe index (the row in dvs_backend_get_keyframes order) of its lowest-id observation
 *            still in the observation table: the first view of its segment in the views CSR.  A landmark no observation names has -1.
 *  Graph     Nodes: all keyframes in table order, R and t as dvs_backend_get_keyframes returns them (x_world = R x + t, unchanged); node
 *            0 is fixed.  Edges k = 0 .. nkf - 2 are the odometry (k, k + 1) with R_z = R_a^T R_b and t_z = R_a^T (t_b - t_a) in double,
 *            every product a left-to-right sum, rvec = Log(R_z) by the Log of the pose-graph residual above, weights odo_w_rot and
 *            odo_w_trans.  Edges nkf - 1 .. are the loops in the order given: (index of the query frame, index of the entry frame, rvec,
 *            tvec, w_rot, w_trans) unchanged — a verified dvs_loop_detect_verified result as it is.
 *  Close     dvs_backend_close_loop builds that graph, solves it on the caller's dvs_pgo handle (same device; the backend owns none)
 *            and, unless the solve FAILED (summary.termination == 2: the map stays byte for byte as it was and the call returns DVS_OK),
 *            (1) makes the keyframe poses the bytes dvs_pgo_get_nodes returns, on the host copy and on the device, (2) runs
 *            dvs_pgo_correct_points_device in place on the landmark table's position column with the device anchors — no position
 *            crosses to the host — and (3), if fusion parameters are given, fuses once per loop in the order given with q = the query
 *            keyframe and E = { k : |k - entry| <= fuse_neighbours, k != q } clipped to the table; each fusion sees the merges of the
 *            one before.  The backend's stream is synchronised before its buffers go to the pose graph and the pose graph's before the
 *            backend touches them again.
 *  Fusion    For a query keyframe q and entry keyframes E (1 .. 64 distinct keyframes, q not among them):
 *            TARGETS are the landmarks in the table named by at least one observation of q; SOURCES are the landmarks in the table named
 *            by at least one observation of a keyframe of E and by none of q.  For a source A and an observation o of q whose landmark
 *            B = o.landmark is in the table, (A, o) is a CANDIDATE iff all of
 *              class(A) == class(o);
 *              c2 > 0 for c = R_q^T (X_A - t_q): the landmark is in front of the camera (the (-1, -1) pixel dvs_associate gives a point
 *                behind the camera never fuses anything);
 *              e = |o.pixel - project(X_A)| < max_reprojection_distance, in the arithmetic of dvs_associate (include/dvslam/
 *                association.hpp reprojection_error: double camera coordinates, float pixel, float difference, double norm);
 *              hamming(desc(A), desc(o)) < max_descriptor_distance.  Both tests are strict.
 *            Every source PROPOSES to the landmark B of its candidate with the smallest (e, o.id).  Every target KEEPS the proposal with
 *            the smallest (e, A.id).  Sources and targets are disjoint and each is in at most one kept pair, so merges never chain.  Of a
 *            kept pair the lower id is the SURVIVOR and the higher id is REMOVED: the survivor gets the sum of the two observation_counts
 *            and the later last_seen and keeps its own position and descriptor; every observation naming the removed landmark names the
 *            survivor instead; the removed row leaves the landmark table by an ordered compaction into the spare table, as in
 *            dvs_backend_prune.  The observation table's other columns, the keyframes' observation_ids and both id counters are
 *            untouched; two observations of one keyframe may then name one landmark, as the reference's association already allows.
 *            Pairs are reported in ascending removed id with their e.  (e, id) is a total order and every minimum is an integer minimum
 *            on the device: there is no tie deviation, and two identical calls on identical maps give identical bytes.
 * Still out of scope: Sim(3), temporal consistency of candidates, re-triangulating the survivor, descriptor re-selection,
 * several GPUs. */
typedef struct dvs_fuse_params {
  double max_descriptor_distance;      /* 50, the backend's */
  double max_reprojection_distance;    /* 5, the backend's */
  int32_t fuse_neighbours;             /* 2; read by dvs_backend_close_loop only; 0 .. 31 */
  int32_t reserved;
} dvs_fuse_params;
typedef struct dvs_fuse_result {
  int32_t n_sources, n_targets;        /* as defined above */
  int32_t n_proposals, n_fused;        /* sources with a candidate / pairs kept */
} dvs_fuse_result;
typedef struct dvs_close_loop_result {
  dvs_pgo_summary summary;
  int32_t n_nodes, n_edges;
  int32_t n_landmarks_moved;           /* landmarks with an anchor >= 0 */
  int32_t reserved;
  dvs_fuse_result fuse;                /* summed over the loops; zero without fusion */
} dvs_close_loop_result;
dvs_status dvs_fuse_default_params(dvs_fuse_params* p);
/* Anchors of all landmarks in ascending id (count-then-capacity: *n is always set; either output may be NULL).  For tests and adapters:
 * dvs_backend_close_loop uses the device array. */
dvs_status dvs_backend_get_anchors(dvs_backend* h, int32_t cap, uint64_t* lm_id, int32_t* anchor_kf, int32_t* n);
/* The graph stated above as the arrays dvs_pgo_set_nodes / dvs_pgo_set_edges take.  Host code only.  Loop arrays: n_loops rows (rvec and
 * tvec 3 doubles each).  Count-then-capacity: *n_nodes = nkf and *n_edges = nkf - 1 + n_loops are set whenever the arguments are valid;
 * every output may be NULL.  DVS_ERR_ARG before anything is written: fewer than 2 keyframes, an unknown frame id, query == entry, a
 * weight not > 0, anything not finite. */
dvs_status dvs_backend_build_pose_graph(dvs_backend* h, int32_t n_loops, const uint64_t* loop_query_frame_id, const uint64_t* loop_entry_frame_id,
                                        const double* loop_rvec, const double* loop_tvec, const double* loop_w_rot, const double* loop_w_trans,
                                        double odo_w_rot, double odo_w_trans, int32_t cap_nodes, int32_t cap_edges, double* R, double* t,
                                        uint8_t* fixed, int32_t* ei, int32_t* ej, double* rvec, double* tvec, double* w_rot, double* w_trans,
                                        int32_t* n_nodes, int32_t* n_edges);
/* CorrectLoop as stated above ("Close").  pgo_params NULL: the defaults; fuse_params NULL: no fusion.  The argument errors of
 * dvs_backend_build_pose_graph, and fusion thresholds that are not finite and > 0, are DVS_ERR_ARG before the map is touched. */
dvs_status dvs_backend_close_loop(dvs_backend* h, dvs_pgo* pgo, int32_t n_loops, const uint64_t* loop_query_frame_id, const uint64_t* loop_entry_frame_id,
                                  const double* loop_rvec, const double* loop_tvec, const double* loop_w_rot, const double* loop_w_trans,
                                  double odo_w_rot, double odo_w_trans, const dvs_pgo_params* pgo_params, const dvs_fuse_params* fuse_params,
                                  dvs_close_loop_result* out);
/* SearchAndFuse as stated above ("Fusion").  params NULL: the defaults.  apply = 0 is a dry run: counts and pairs, the map not modified.
 * survivor_id / removed_id / err: the kept pairs in ascending removed id, each nullable; *n_pairs (nullable) = their number.  If any of
 * the three is given and cap_pairs is too small: DVS_ERR_CAPACITY, nothing applied.  DVS_ERR_ARG before any device work: an unknown frame
 * id, q in the entry list, a repeated entry, n_entry outside 1 .. 64, thresholds not finite or not > 0. */
dvs_status dvs_backend_fuse(dvs_backend* h, uint64_t query_frame_id, const uint64_t* entry_frame_ids, int32_t n_entry, const dvs_fuse_params* params,
                            int32_t apply, dvs_fuse_result* out, int32_t cap_pairs, uint64_t* survivor_id, uint64_t* removed_id, double* err,
                            int32_t* n_pairs);

/* ---- Global BA of the map --------------------------------------------------------------------------------------------------------
 * The step after CorrectLoop: every keyframe and every landmark of the map refined by dvs_ba_solve_global (B3 above) on the caller's
 * dvs_ba handle (same device; the backend owns none, as dvs_backend_close_loop takes a dvs_pgo).  PARITY UNPINNED: the reference has no
 * global BA; the rule is this library's own, restated over the getters' arrays in tests/global_ba_ref.py.
 *   Cameras       all keyframes in table order, converted by dvs_ba_pose_from_rt; keyframe 0 is the fixed gauge, as SlidingWindowBA
 *                 fixes its first.
 *   Landmarks     all rows in ascending id, positions float -> double, none fixed.
 *   Observations  all rows of the observation table, in table order, whose landmark is in the table (the obs_lm_index >= 0 rule of
 *                 dvs_backend_get_window), pixels float -> double; the observations of a landmark with fewer than two such rows are left
 *                 out.  Limitation: a landmark left without observations keeps its position bytes — nothing re-triangulates it.
 *   Settings      the backend's fx .. cy, sigma 1.0, Huber 1.345.
 *   Result        applied through dvs_backend_apply_optimized (keyframes 1 .., the landmarks with observations; positions rounded to
 *                 float once) if and only if summary.ba.termination == 0.  Otherwise the map stays byte for byte as it was and the
 *                 call still returns DVS_OK with the summary.  Fewer than 2 keyframes or no usable observation: DVS_ERR_ARG before
 *                 the map is touched.
 *   Data path     the problem is assembled on the HOST from one read-back per table column, as the per-keyframe BA cycle does through
 *                 dvs_backend_get_window; handing the tables over on the device is not built.
 * n_left_out counts the observation-table rows that are not in the problem. */
typedef struct dvs_backend_gba_result {
  dvs_ba_global_summary summary;
  int32_t n_cameras, n_landmarks, n_observations, n_left_out;
} dvs_backend_gba_result;
dvs_status dvs_backend_global_ba(dvs_backend* h, dvs_ba* ba, const dvs_ba_global_params* params /* NULL: defaults */, dvs_backend_gba_result* out);

/* ======================================= Tracking against the map ================================= */
/* A frame's keypoints matched against the landmarks of the map and its pose refined on those 3D-2D pairs (csrc/map_track.hip;
 * INTEGRATION.md "Tracking against the map"): what ORB-SLAM calls TrackLocalMap — SearchByProjection, then PoseOptimization (Mur-Artal,
 * Montiel, Tardos 2015, section V-D), as published ideas.  The reference's front end is odometry only, so there is no reference interface
 * to pin: PARITY UNPINNED, the rule is the library's own, stated here in full and restated in numpy in tests/map_track_ref.py.  Integer
 * outputs and the stage-1 doubles are compared bit for bit; the refinement calls sin / cos / sqrt and is compared through its inlier flags
 * and its cost.
 * Poses at the interface are camera-to-world as the tracker's and the backend's (X_w = R X_c + t, R 9 row-major doubles).  Inside,
 * R_cw = R^T and t_cw[i] = -((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]).
 *  Inputs    n_lm landmarks — float xyz[3], uint8 desc[32], int64 id in ascending order (a row index stands for the id where no id array
 *            is given) —, n_kp keypoints — dvs_keypoint, uint8 desc[32] —, the prior pose, the parameters.
 *  Stage 1   projection, one landmark on its own, FP64, only + - * /, every expression left to right as written, no contraction.
 *            X = the float position widened; c[i] = ((R_cw[3i] * X0 + R_cw[3i + 1] * X1) + R_cw[3i + 2] * X2) + t_cw[i];
 *            u = fx * c0 / c2 + cx, v = fy * c1 / c2 + cy.  VISIBLE iff min_z < c2 && c2 < max_z && 0 <= u && u < cols && 0 <= v &&
 *            v < rows, compared as doubles.  A landmark that is not visible reports u = v = 0.
 *  Stage 2   window search.  A keypoint is BINNED iff 0 <= x < cols && 0 <= y < rows (as floats) and 0 <= octave < n_levels; its cell
 *            is ((int)x / cell, (int)y / cell) of a grid of ceil(cols / cell) x ceil(rows / cell) square cells, cells in row-major
 *            order, the keypoints of a cell in ascending index (a stable counting sort).  A keypoint that is not binned is never
 *            matched; the host-pointer form refuses it (DVS_ERR_ARG), the device-pointer forms count it in n_unbinned.
 *            A binned keypoint k is a CANDIDATE of a visible landmark j iff |(double)x_k - u| <= radius && |(double)y_k - v| <= radius.
 *            Only the cells that overlap the window are visited; the outcome does not depend on `cell`.  d = hamming(desc_j, desc_k);
 *            best = the candidate with the smallest (d, k); d_second = the smallest d among the OTHER candidates (-1 if none).  The
 *            landmark PROPOSES to best iff d_best < max_hamming (strict, as in the backend) and (there is no other candidate, or
 *            ratio_pct <= 0, or d_best * 100 < ratio_pct * d_second — integers).
 *  Stage 3   one-to-one.  Every keypoint KEEPS the proposal with the smallest (d, landmark row) — rows ascend with the id; an integer
 *            minimum on the device, so there is no tie deviation.  A landmark that loses stays unmatched: there is no second round.
 *  Stage 4   pose refinement on the kept pairs in keypoint order: X_i the landmark position widened, p_i = (x, y) of the keypoint widened,
 *            s2_i = level_sigma2[octave].  With c = R_cw X_i + t_cw (as in stage 1): e_i = p_i - (fx c0 / c2 + cx, fy c1 / c2 + cy),
 *            chi_i = (e_i . e_i) / s2_i; a pair with c2 <= 0 has chi_i = +infinity and adds nothing to any sum.  A pair whose X_i is not
 *            finite has no finite c2 and is treated the same way: a permanent outlier.  A pair whose p_i is not finite ends the
 *            refinement as soon as it enters a sum: DEGENERATE, the prior's bytes, all flags 0.  Parameters
 *            delta = (omega, upsilon): R_cw <- Exp(omega) R_cw, t_cw <- Exp(omega) t_cw + upsilon, Exp by Rodrigues' formula
 *            (|omega| < 1e-12: I + [omega]x); the camera point's Jacobian is [-[c]x | I].  Four rounds of ten Gauss-Newton steps
 *            H delta = b, H = sum w_i J_i^T J_i / s2_i, b = sum w_i J_i^T e_i / s2_i, no step control.  Rounds 0 and 1: w_i =
 *            sqrt(chi2_gate / chi_i) where chi_i > chi2_gate, else 1 (Huber with delta^2 = chi2_gate); rounds 2 and 3: w_i = 1.  The sums
 *            run over the pairs currently flagged inlier — all of them before round 0 —; after every round ALL pairs are reclassified,
 *            outliers included: inlier iff chi_i <= chi2_gate at the round's last pose.  The 6 x 6 system is solved by Cholesky in FP64
 *            by one lane; the 27 sums and the cost are formed in one fixed order (pair i on lane i mod 256, the lanes added in a fixed order), so
 *            two identical calls give identical bytes.  A pivot <= 1e-10 * max_diag(H), or anything not finite, ends the refinement.
 *  Outcome   status 0 OK; 1 FEW_MATCHES: fewer than min_matches kept pairs, no refinement is run; 2 FEW_INLIERS: fewer than min_inliers
 *            inliers after round 3; 3 DEGENERATE.  For every status but 0 the returned pose is the prior, byte for byte.  With status 0
 *            it is R = R_cw^T, t[i] = -((R_cw[i] * t_cw[0] + R_cw[3 + i] * t_cw[1]) + R_cw[6 + i] * t_cw[2]), converted once at the end.
 *            cost = sum of chi_i over the final inliers at the final pose (0 unless the four rounds ran).  Every status is DVS_OK.
 * All four rounds run inside ONE kernel of one call; no host decision is taken between iterations; one 128-byte record comes back.
 * Out of scope: a predicted octave (the observation table has none), several GPUs.  The viewing-angle and distance gates and the descriptor
 * re-selection are "Landmark refresh" below.  (A frame whose prior is not within `radius` of the truth is what "Relocalisation" below is for.) */
typedef struct dvs_maptrack dvs_maptrack;
#define DVS_MAPTRACK_MAX_LEVELS 16
enum { DVS_MAPTRACK_OK = 0, DVS_MAPTRACK_FEW_MATCHES = 1, DVS_MAPTRACK_FEW_INLIERS = 2, DVS_MAPTRACK_DEGENERATE = 3 };
typedef struct dvs_maptrack_params {
  int32_t rows, cols;                  /* 1..16384 each */
  double fx, fy, cx, cy;               /* finite, fx, fy > 0 */
  double min_z, max_z;                 /* 0.05 / 20.0 metres; 0 <= min_z < max_z, finite */
  double radius;                       /* 15.0 pixels; finite, >= 0 */
  int32_t cell;                        /* 32; 1..16384, and at most 2^20 cells */
  int32_t max_hamming;                 /* 50; 0..257 */
  int32_t ratio_pct;                   /* 90; <= 0 switches the ratio test off; <= 100000 */
  int32_t reserved0;
  double chi2_gate;                    /* 5.991; finite, > 0 */
  int32_t min_matches;                 /* 15; >= 3 */
  int32_t min_inliers;                 /* 10; >= 0 */
  int32_t n_levels;                    /* 8; 1..DVS_MAPTRACK_MAX_LEVELS */
  int32_t reserved1;
  double level_sigma2[DVS_MAPTRACK_MAX_LEVELS];   /* the extractor's sigma2 table (dvs_orb_get_tables) widened; the first n_levels finite, > 0 */
} dvs_maptrack_params;
typedef struct dvs_maptrack_result {   /* 128 bytes */
  double R[9], t[3];                   /* the refined pose with status 0, else the prior's bytes */
  double cost;
  int32_t status;                      /* DVS_MAPTRACK_* */
  int32_t n_visible, n_proposed;       /* landmarks visible / that proposed */
  int32_t n_matches;                   /* kept pairs (refine_device: the correspondences given) */
  int32_t n_inliers;                   /* inliers of the last classification (0 with FEW_MATCHES and DEGENERATE) */
  int32_t n_unbinned;                  /* keypoints outside the image or the octave table (device-pointer forms) */
} dvs_maptrack_result;
/* the defaults above, level_sigma2 = the float table of scale factor 1.2 over 8 levels widened; rows / cols / intrinsics stay zero */
void dvs_maptrack_default_params(dvs_maptrack_params* p);
/* DVS_ERR_ARG for parameters outside the ranges above, before any device work; then DVS_ERR_NO_DEVICE without a gfx950 (no CPU fallback).
 * The handle works on HIP's legacy default stream until dvs_maptrack_set_stream.  Not thread-safe; buffers grow with the largest call. */
dvs_status dvs_maptrack_create(const dvs_maptrack_params* params, int32_t device, dvs_maptrack** out);
void dvs_maptrack_destroy(dvs_maptrack* h);
dvs_status dvs_maptrack_set_stream(dvs_maptrack* h, void* hip_stream);   /* synchronises the old stream first */
/* Stages 1-3 on device arrays.  d_lm_id may be NULL (ids = rows); descriptor arrays 8-byte aligned; R9 / t3 host, finite.  result NULL: the
 * call does not synchronise; otherwise it waits and fills the counts (pose = the prior, status 0, cost 0, n_inliers 0). */
dvs_status dvs_maptrack_search_device(dvs_maptrack* h, const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id, int32_t n_lm,
                                      const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp, const double* R9, const double* t3,
                                      dvs_maptrack_result* result);
/* Stage 4 alone — PoseOptimization on explicit correspondences: d_X n x 3 doubles, d_px n x 2 doubles, d_octave n int32 (an octave outside
 * the table makes its pair a permanent outlier).  n_matches = n; fewer than min_matches is FEW_MATCHES.  Synchronises. */
dvs_status dvs_maptrack_refine_device(dvs_maptrack* h, const double* d_X, const double* d_px, const int32_t* d_octave, int32_t n, const double* R9,
                                      const double* t3, dvs_maptrack_result* result);
/* Stages 1-4 in one call: the search's launches, then the one refinement kernel, which also gathers the kept pairs.  Synchronises. */
dvs_status dvs_maptrack_track_device(dvs_maptrack* h, const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id, int32_t n_lm,
                                     const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp, const double* R9, const double* t3,
                                     dvs_maptrack_result* result);
/* the same with host pointers (lm_id may be NULL); an unbinned keypoint and ids that do not ascend strictly are DVS_ERR_ARG */
dvs_status dvs_maptrack_track(dvs_maptrack* h, const float* lm_xyz, const uint8_t* lm_desc, const int64_t* lm_id, int32_t n_lm, const dvs_keypoint* kps,
                              const uint8_t* desc, int32_t n_kp, const double* R9, const double* t3, dvs_maptrack_result* result);
/* The last call's per-keypoint arrays (each nullable, count-then-capacity: *n = the last call's n_kp is always set): the landmark row kept
 * (-1: none), its id, the distance (-1: none) and whether the pair ended as an inlier (all 0 unless status is 0 or 2).  After
 * dvs_maptrack_refine_device the rows are the correspondences: lm_row[i] = lm_id[i] = i, dist 0. */
dvs_status dvs_maptrack_get_matches(dvs_maptrack* h, int32_t cap, int32_t* lm_row, int64_t* lm_id, int32_t* dist, uint8_t* inlier, int32_t* n);
/* dvs_maptrack_track_device with the backend's landmark table as it stands — position, descriptor and id columns handed over on the device,
 * nothing of them crosses to the host; the map is not modified.  Same device for both handles; the backend's stream is synchronised first. */
dvs_status dvs_backend_track_frame(dvs_backend* h, dvs_maptrack* mt, const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp, const double* R9,
                                   const double* t3, dvs_maptrack_result* result);
/* After a dvs_tracker_track: the last frame's depth-filtered keypoints and descriptors where the tracker left them in HBM, with the prior
 * R_, t_, through dvs_backend_track_frame.  With apply != 0 and status 0 the refined pose replaces R_, t_, so the next frame's odometry
 * composes on it (the motion mask's ring keeps the poses it recorded).  DVS_ERR_EMPTY before the first frame; the three handles
 * are on one device, and mt's size and intrinsics are the caller's to make the tracker's.  Strictly opt-in: a tracker on which it is never called allocates and launches nothing it did not before. */
dvs_status dvs_tracker_track_map(dvs_tracker* h, dvs_backend* backend, dvs_maptrack* mt, int32_t apply, dvs_maptrack_result* result);
/* that set, for tests and adapters (kps / desc nullable, `cap` rows; *n = rows available) */
dvs_status dvs_tracker_get_filtered_features(dvs_tracker* h, dvs_keypoint* kps, uint8_t* desc, int32_t cap, int32_t* n);

/* ======================================= Covisibility ================================= */
/* The covisibility graph of the map the backend keeps on the device (csrc/covisibility.hip; INTEGRATION.md "Covisibility"): keyframes as
 * nodes, the number of landmarks two keyframes both observe as the edge weight — what ORB-SLAM organises its local map and its local BA
 * around (Mur-Artal, Montiel, Tardos 2015, sections III-D and VI-D), as published ideas.  PARITY UNPINNED: the reference has no counterpart;
 * the rule is the library's own, defined over the tables as the getters return them, stated here in full and restated with Python sets in
 * tests/covisibility_ref.py.
 *  Observes   Keyframe k (index in table order) observes landmark L iff the landmark table holds L and at least one observation row has
 *             kf == k (its frame_id is keyframe k's) and landmark_id == L.  S_k is the set of those landmarks.  Two rows of one keyframe
 *             naming one landmark count once (this happens after fusion, and the reference's association allows it); a row naming a
 *             landmark the table does not hold counts nowhere.
 *  Weights    W[a][b] = |S_a n S_b| for a != b, W[a][a] = |S_a|; int32, symmetric by construction.
 *  Neighbours N(a; theta) = the keyframes b != a with W[a][b] >= theta, ordered by weight descending, then index ascending; theta >= 1.
 *  Local set  of a reference keyframe r with (theta, max_neighbours): the FREE keyframes are r and the first max_neighbours of
 *             N(r; theta); the LOCAL LANDMARKS U are the union of S_k over the free keyframes, in ascending id.
 *  Fixed      (BA only) the keyframes c that are not free and have f_c = |S_c n U| >= 1, ordered by (f_c descending, index ascending),
 *             the first max_fixed of them.  If that leaves no fixed keyframe, the free keyframe of lowest index is marked fixed: the
 *             gauge, as SlidingWindowBA fixes its first.
 *  Window     keyframes (free and fixed) in ascending table index, each with a `fixed` byte and its weight to r (W[r][k]; for r itself
 *             W[r][r]); landmarks U; observations = the rows of the observation table, in table order, whose keyframe is in the window,
 *             whose landmark is in U and that are the FIRST row in table order of their (keyframe, landmark) pair — dvs_ba_solve_device
 *             takes a landmark at most once per camera.  The later rows of such pairs are counted in n_left_out.  obs_lm_index is the
 *             landmark's row in U and is never -1.
 * Every quantity is an integer and every order is total: there is no tie deviation, two identical calls on identical maps give identical
 * bytes, and no call but dvs_backend_local_ba modifies the map.
 * Limit: the row kernel keeps one 4-byte counter per keyframe in LDS, 32 KiB at most (four workgroups per compute unit); a map of more
 * than DVS_COVIS_MAX_KEYFRAMES keyframes is refused with DVS_ERR_CAPACITY by every call of this section.
 * DVS_ERR_ARG before any device work: min_weight < 1, max_neighbours outside 0..62, max_fixed outside 0..63, max_neighbours + 1 +
 * max_fixed > 64 (the device solver's camera limit), ba_max_iterations < 1, an unknown ref_frame_id.
 * Out of scope: covisibility edges in the pose graph, a cached graph, scale and viewing-angle conditions, several GPUs.  Removing redundant
 * keyframes is the next section, "Keyframe culling". */
#define DVS_COVIS_MAX_KEYFRAMES 8192
typedef struct dvs_covis_params {
  int32_t min_weight;          /* 15: theta */
  int32_t max_neighbours;      /* 10: with r, 11 free cameras — inside the in-LDS solver's default window of 16 */
  int32_t max_fixed;           /* 32 */
  int32_t ba_max_iterations;   /* 20 (SlidingWindowBA's); read by dvs_backend_local_ba only */
} dvs_covis_params;
void dvs_covis_default_params(dvs_covis_params* p);
/* The whole graph, count-then-capacity: *n_kf and *n_nb (the total length of all neighbour lists at min_weight) are always set.
 * weights: n_kf x n_kf row-major, nullable.  Neighbour lists as CSR, each array nullable: nb_offsets n_kf + 1, nb_index / nb_weight
 * *n_nb entries.  DVS_ERR_CAPACITY if an array is given and cap_kf < *n_kf (weights, nb_offsets) or cap_nb < *n_nb (nb_index, nb_weight). */
dvs_status dvs_backend_covisibility(dvs_backend* h, int32_t min_weight, int32_t cap_kf, int64_t cap_nb, int32_t* weights, int64_t* nb_offsets,
                                    int32_t* nb_index, int32_t* nb_weight, int32_t* n_kf, int64_t* n_nb);
/* The local window of keyframe ref_frame_id: dvs_backend_get_window's outputs (each nullable, count-then-capacity: the three counts are
 * always set) plus kf_fixed, kf_weight and *n_left_out (nullable).  params NULL: the defaults. */
dvs_status dvs_backend_get_local_window(dvs_backend* h, uint64_t ref_frame_id, const dvs_covis_params* params, int32_t cap_kf, int32_t cap_obs,
                                        int32_t cap_lm, uint64_t* kf_frame_id, double* kf_R, double* kf_t, uint8_t* kf_fixed, int32_t* kf_weight,
                                        int32_t* n_kf, float* obs_px, uint64_t* obs_lm_id, int32_t* obs_class, uint64_t* obs_frame_id,
                                        int32_t* obs_lm_index, int32_t* n_obs, uint64_t* lm_id, int32_t* lm_class, float* lm_xyz, int32_t* n_lm,
                                        int32_t* n_left_out);
/* Local BA: the local window refined on the caller's dvs_ba handle (same device), as dvs_backend_global_ba refines the whole map.
 *   Cameras       the window's keyframes in its order through dvs_ba_pose_from_rt, pose_fixed = the window's fixed bytes.
 *   Landmarks     the rows of U that keep at least two of the window's observations, in ascending id, float -> double, none fixed.
 *   Observations  the window's, in its order, pixels float -> double, without those of a landmark with fewer than two of them
 *                 (counted in n_dropped), as global BA drops them.
 *   Settings      the backend's fx .. cy, sigma 1.0, Huber 1.345; dvs_ba_solve_device with ba_max_iterations and SlidingWindowBA's
 *                 tolerances 1e-6 / 1e-10 / 1e-8.  dvs_ba_set_device_window is never called: a caller who raises max_neighbours above
 *                 15 raises the window on their own handle; DVS_ERR_UNSUPPORTED from the solver is passed on.
 *   Result        applied through dvs_backend_apply_optimized — the keyframes that are not fixed and the problem's landmarks, positions
 *                 rounded to float once — if and only if summary.termination == 0.  Otherwise the map stays byte for byte as it was and
 *                 the call still returns DVS_OK with the summary.  No camera that is not fixed, or no observation left: DVS_ERR_ARG
 *                 before the map is touched. */
typedef struct dvs_backend_lba_result {
  dvs_ba_summary summary;
  int32_t n_cameras, n_fixed, n_landmarks, n_observations, n_left_out, n_dropped;
} dvs_backend_lba_result;
dvs_status dvs_backend_local_ba(dvs_backend* h, dvs_ba* ba, uint64_t ref_frame_id, const dvs_covis_params* params /* NULL: defaults */,
                                dvs_backend_lba_result* out);
/* dvs_backend_track_frame against the local map of keyframe ref_frame_id: U's position, descriptor and id columns are compacted on the
 * device in ascending id into the backend's scratch and handed to dvs_maptrack_track_device as dvs_backend_track_frame hands over the whole
 * table; nothing of the map crosses to the host.  dvs_maptrack_get_matches then reports rows of U, and the ids identify them.  max_fixed
 * and ba_max_iterations are checked and not used. */
dvs_status dvs_backend_track_frame_local(dvs_backend* h, dvs_maptrack* mt, uint64_t ref_frame_id, const dvs_covis_params* params /* NULL: defaults */,
                                         const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp, const double* R9, const double* t3,
                                         dvs_maptrack_result* result);

/* ======================================= Keyframe culling ================================= */
/* Redundant keyframes leave the map the backend keeps on the device (csrc/kf_cull.hip; INTEGRATION.md "Keyframe culling"): a keyframe goes
 * when almost everything it sees is seen well enough by others — the idea of ORB-SLAM's KeyFrameCulling (Mur-Artal, Montiel, Tardos 2015,
 * section VI-E) as published, not its code.  PARITY UNPINNED: the reference has no counterpart; the rule is the library's own, defined over
 * the tables as the getters return them BEFORE the call, stated here in full and restated with Python sets in tests/keyframe_culling_ref.py.
 * Observes, S_k and the neighbour lists N(a; theta) are exactly those of "Covisibility": two rows of one keyframe naming one landmark count
 * once, and a row naming a landmark the table does not hold counts nowhere.
 *  Observers  c(L) = the number of keyframes that observe L.
 *  Redundancy for keyframe k: n_k = |S_k|; R_k = the number of L in S_k with c(L) - 1 >= min_observers; k is REDUNDANT iff n_k >= 1 and
 *             100 * R_k > redundancy_percent * n_k, evaluated in 64-bit integers with a strict >.
 *  Protected  never culled: the keyframe at index 0 (the gauge of sliding, local and global BA); the last keep_recent keyframes in table
 *             order; every keyframe named in protected_frame_ids; ref_frame_id itself in local scope.
 *  Scope      local == 0: every keyframe is in scope and ref_frame_id is not read.  local != 0: only the keyframes of N(ref; min_weight)
 *             are in scope — the whole list, not truncated by any max_neighbours.
 *  Candidates the keyframes that are in scope and not protected.
 *  Walk       SEQUENTIAL, which is what makes the rule safe: candidates are visited in ascending table index; at its turn k is tested with
 *             the CURRENT c(.); if it is redundant it is CULLED and c(L) -= 1 for every L in S_k before the next candidate is tested.  The
 *             walk stops early when max_cull > 0 and that many keyframes have been culled.  A one-shot test of all candidates against the
 *             initial counts is NOT this rule: it can remove every observer of a landmark.
 *  Report     per keyframe in table order before the call: kf_observed = n_k; kf_redundant = R_k from the INITIAL counts, for every
 *             keyframe whatever its state; kf_state: 1 = protected, else 0 = out of scope, else 3 = culled, else 2 = kept.
 *             culled_frame_id: the culled keyframes' frame ids in ascending index (the first out->n_culled entries).
 *  Apply      (apply != 0 and at least one keyframe culled)
 *             Observation rows  every row whose keyframe is culled leaves the observation table by ordered compaction: the other rows keep
 *                               their order and every column.
 *             Landmarks         observation_count drops by the number of removed rows naming the landmark, never below 0.  With
 *                               drop_orphans != 0 a landmark that had at least one row before the call and has none after it leaves the
 *                               landmark table, again by ordered compaction.  Position, descriptor and last_seen of those that stay are
 *                               untouched.
 *             Keyframes         the culled keyframes leave the keyframe list and the poses, order kept; the kept keyframes'
 *                               observation_ids are untouched; both id counters are untouched.
 *             If nothing is culled, or apply == 0, the map stays byte for byte as it was.
 * Every quantity is an integer and every order is total: two identical calls on identical maps give identical bytes.
 * DVS_ERR_ARG before any device work: min_observers < 1, redundancy_percent outside 0..99, min_weight < 1, keep_recent < 0, max_cull < 0,
 * n_protected < 0, an unknown protected or (local scope) reference frame id.  DVS_ERR_CAPACITY: more than DVS_COVIS_MAX_KEYFRAMES keyframes
 * when local != 0 (the row kernel's limit); count-then-capacity as everywhere: *n_kf is always set, and if an output array is given with
 * cap_kf < *n_kf nothing is computed and nothing is applied.  An empty map returns DVS_OK with zeros.
 * Out of scope: scale and viewing-angle conditions (the observation table has no octave), time-spacing conditions, removing entries from a
 * dvs_loop database (the caller does that with culled_frame_id), a cached graph, several GPUs. */
typedef struct dvs_cull_params {
  int32_t min_observers;       /* 3 */
  int32_t redundancy_percent;  /* 90 */
  int32_t min_weight;          /* 15: theta; read only when local != 0 */
  int32_t local;               /* 0 */
  int32_t keep_recent;         /* 2 */
  int32_t max_cull;            /* 0: no limit */
  int32_t drop_orphans;        /* 1 */
  int32_t reserved;
} dvs_cull_params;             /* 32 bytes */
typedef struct dvs_cull_result {
  int32_t n_keyframes, n_candidates, n_redundant_initial, n_culled;   /* n_redundant_initial: over every keyframe, whatever its state */
  int32_t n_observations_removed, n_landmarks_removed, reserved[2];   /* what apply removes, also in a dry run */
} dvs_cull_result;             /* 32 bytes */
void dvs_cull_default_params(dvs_cull_params* p);
/* out and the four arrays are nullable; each array takes *n_kf entries (culled_frame_id: out->n_culled of them are written). */
dvs_status dvs_backend_cull_keyframes(dvs_backend* h, uint64_t ref_frame_id, const dvs_cull_params* params /* NULL: defaults */,
                                      const uint64_t* protected_frame_ids, int32_t n_protected, int32_t apply, dvs_cull_result* out,
                                      int32_t cap_kf, uint64_t* culled_frame_id, int32_t* kf_observed, int32_t* kf_redundant,
                                      uint8_t* kf_state, int32_t* n_kf);

/* ======================================= Landmark refresh ================================= */
/* A landmark's descriptor re-selected from all its views, its viewing geometry, and map tracking gated by that geometry
 * (csrc/landmark_refresh.hip, csrc/map_track.hip; INTEGRATION.md "Landmark refresh"): what ORB-SLAM runs per keyframe as
 * ComputeDistinctiveDescriptors and UpdateNormalAndDepth and tests in isInFrustum (Mur-Artal, Montiel, Tardos 2015, sections III-C and V-D),
 * as published ideas.  PARITY UNPINNED: the reference has no counterpart; the rule is the library's own, defined over the tables as the
 * getters return them, stated here in full and restated in numpy and Python sets in tests/landmark_refresh_ref.py.  Everything is opt-in:
 * a program that never calls this section computes and allocates what it did before.
 *  Views      The views of landmark row s are the observation rows whose landmark_id is the row's id, in observation-table order (the
 *             obs_offsets / obs_ids segment of dvs_backend_get_landmarks).  Two rows of one keyframe naming one landmark are two views.
 *  Descriptor integers only.  With n views of descriptors d_0 .. d_{n-1}: D[i][j] = hamming(d_i, d_j), D[i][i] = 0 included; med_i = the
 *             element at index (n - 1) / 2 (integer division) of row i sorted ascending; the CHOSEN view is the one with the smallest
 *             (med_i, i): the first view in table order wins ties.  n == 0 or n < min_views: the landmark keeps its bytes.  No upper
 *             limit on n.
 *  Geometry   FP64, no contraction, every expression left to right as written.  View p of keyframe index k COUNTS iff k is a keyframe of
 *             the map and r is finite and > 0, with C = kf_t[k], X = the float position widened, d = X - C,
 *             r = sqrt((d0 * d0 + d1 * d1) + d2 * d2).  With the m counted views in view order: normal[c] = (sum of d[c] / r) / m, each
 *             component summed sequentially from 0.0 and NOT re-normalised; dmin = min r, dmax = max r.  m == 0: normal = 0, dmin = dmax = 0.
 *  Gates      stage 1 of "Tracking against the map", before the projection; only + - * / and comparisons.  O = the prior's t, p = X - O,
 *             q = (p0 * p0 + p1 * p1) + p2 * p2, s = (p0 * N0 + p1 * N1) + p2 * N2, a = dmin / range_factor, b = dmax * range_factor,
 *             cc = cos_min * cos_min.  A landmark with m > 0 is GATED OUT, and counted at the FIRST test that holds, in this order:
 *             near q < a * a; far q > b * b; back-facing s < 0; angle s * s < cc * q.  A gated landmark is treated exactly as one that is
 *             not visible (u = v = 0, it proposes nothing, it is not in n_visible); it is counted whether or not it would have been
 *             visible.  A landmark with m == 0 passes and is counted nowhere.
 *  Scope      use_scope == 0: every landmark row.  use_scope != 0: the landmarks keyframe scope_frame_id observes ("Covisibility": S_k).
 * cos_min in [0, 1], range_factor >= 1 and finite, min_views >= 1; an unknown scope_frame_id: DVS_ERR_ARG before any device work.  The
 * defaults — cos_min 0.5 (60 degrees), range_factor 2.0, min_views 1 — are usual values, never fitted to a sensor.
 * The selection is integers and total orders: two identical calls give identical bytes.  Nothing is cached between calls: every call
 * rebuilds the views from the tables as they stand, as "Covisibility" does.
 * Names: the gated calls on a dvs_maptrack handle carry the prefix dvs_mapgate_, not dvs_maptrack_: tests/test_map_track_cpu.py pins the
 * exact set of dvs_maptrack_ functions, as tests/test_loop_cpu.py does for dvs_loop_.
 * Out of scope: an octave column and octave prediction from distance, cached geometry or new landmark columns, gates in relocalisation,
 * fusion, dvs_backend_track_frame_local and the association of dvs_backend_add_keyframe, a policy that calls the refresh, several GPUs. */
typedef struct dvs_lm_refresh_params {
  int32_t update_descriptors;  /* 1; 0: a dry run that only fills the result */
  int32_t min_views;           /* 1 */
  int32_t use_scope;           /* 0 */
  int32_t reserved;
  uint64_t scope_frame_id;     /* read only when use_scope != 0 */
} dvs_lm_refresh_params;       /* 24 bytes */
typedef struct dvs_lm_refresh_result {
  int32_t n_in_scope;          /* landmark rows in scope */
  int32_t n_changed;           /* of them: n >= max(min_views, 1) and the chosen view's bytes differ from the landmark's */
  int32_t n_without_views;     /* of them: n == 0 */
  int32_t max_views;           /* the largest n in scope */
} dvs_lm_refresh_result;       /* 16 bytes */
typedef struct dvs_maptrack_gates { double cos_min, range_factor; } dvs_maptrack_gates;   /* 0.5, 2.0 */
void dvs_lm_refresh_default_params(dvs_lm_refresh_params* p);
void dvs_mapgate_default_gates(dvs_maptrack_gates* g);
/* Builds the views, selects the view of every landmark in scope and (update_descriptors != 0) writes the chosen descriptor into the landmark
 * table in place; nothing else in the map changes, and with n_changed == 0 no byte does.  params NULL: the defaults; result nullable. */
dvs_status dvs_backend_refresh_landmarks(dvs_backend* h, const dvs_lm_refresh_params* params, dvs_lm_refresh_result* result);
/* A dry run over the whole table, count-then-capacity (*n = landmark rows is always set; DVS_ERR_CAPACITY, nothing written, if an array is
 * given and cap < *n), every output nullable, the map never modified: normal n x 3, range n x 2 (dmin, dmax), n_counted = m, best_obs_id =
 * the chosen view's observation id (UINT64_MAX where n == 0), best_median = its med_i (-1 where n == 0) — chosen as with min_views 1. */
dvs_status dvs_backend_get_landmark_geometry(dvs_backend* h, int32_t cap, double* normal, double* range, int32_t* n_counted, uint64_t* best_obs_id,
                                             int32_t* best_median, int32_t* n);
/* dvs_maptrack_search_device / dvs_maptrack_track_device with the gates: d_lm_normal n_lm x 3 doubles, d_lm_range n_lm x 2 doubles,
 * d_lm_ncounted n_lm int32 (device, 8 / 8 / 4-byte aligned), gates NULL: the defaults.  The ungated calls are untouched. */
dvs_status dvs_mapgate_search_device(dvs_maptrack* h, const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id, int32_t n_lm,
                                     const double* d_lm_normal, const double* d_lm_range, const int32_t* d_lm_ncounted,
                                     const dvs_maptrack_gates* gates, const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp,
                                     const double* R9, const double* t3, dvs_maptrack_result* result);
dvs_status dvs_mapgate_track_device(dvs_maptrack* h, const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id, int32_t n_lm,
                                    const double* d_lm_normal, const double* d_lm_range, const int32_t* d_lm_ncounted,
                                    const dvs_maptrack_gates* gates, const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp,
                                    const double* R9, const double* t3, dvs_maptrack_result* result);
/* the last call's gate counts: near, far, back-facing, angle (all 0 after an ungated call); synchronises */
dvs_status dvs_mapgate_get_counts(dvs_maptrack* h, int32_t out[4]);
/* dvs_backend_track_frame with the gates: the geometry of the table as it stands is computed into the backend's scratch (the views and one
 * sequential FP64 walk per landmark), then dvs_mapgate_track_device runs; the map is not modified. */
dvs_status dvs_backend_track_frame_gated(dvs_backend* h, dvs_maptrack* mt, const dvs_maptrack_gates* gates /* NULL: defaults */, const dvs_keypoint* d_kps,
                                         const uint8_t* d_desc, int32_t n_kp, const double* R9, const double* t3, dvs_maptrack_result* result);
/* dvs_tracker_track_map through dvs_backend_track_frame_gated */
dvs_status dvs_tracker_track_map_gated(dvs_tracker* h, dvs_backend* backend, dvs_maptrack* mt, const dvs_maptrack_gates* gates, int32_t apply,
                                       dvs_maptrack_result* result);

/* ======================================= Landmark culling ================================= */
/* What a frame learns while it is tracked against the map reaches the map: two counters per landmark, recorded by the map-tracking calls
 * of the backend, and a cull that removes the landmarks the frames keep predicting and never find — a chair that was moved — and the
 * landmarks only their creating keyframe ever saw (csrc/lm_cull.hip, csrc/map_track.hip; INTEGRATION.md "Landmark culling"): the ideas of
 * ORB-SLAM's mnVisible / mnFound and MapPointCulling (Mur-Artal, Montiel, Tardos 2015, section VI-B) as published, not its code.  PARITY
 * UNPINNED: the reference has no counterpart; the rule is the library's own, stated here in full and restated with dicts and Python sets in
 * tests/landmark_culling_ref.py.  Everything is integers and total orders: the device matches the restatement bit for bit.  Everything is
 * opt-in: a program that never calls this section allocates, launches and computes what it did before.
 *  Statistics two int32 counters per landmark, visible and found, kept in a side table of the handle joined to the landmark table BY ID; the
 *             landmark table has no new column.  Every call of this section first ALIGNS the side table to the landmark table as it
 *             stands: an id the statistics hold keeps its counters, an id they do not hold starts at 0 / 0, the statistics of ids no longer
 *             in the table are dropped.  Landmark ids only grow, so an id never comes back with another landmark's counters.  After a
 *             fusion the survivor keeps its own counters and the removed id's are dropped; they are not merged.  dvs_backend_reset empties
 *             the statistics and leaves the switch as set.  Nothing is cached about "the map did not change": every call aligns.
 *  Recording  off until dvs_backend_set_tracking_stats(h, 1).  While it is on, dvs_backend_track_frame, dvs_backend_track_frame_gated and
 *             dvs_backend_track_frame_local (and so dvs_tracker_track_map and dvs_tracker_track_map_gated) end by recording their own
 *             outcome, before they return.  With j over the rows handed to the tracker — the whole table, or the local map U, where the
 *             id decides, not the row: if the result's status != DVS_MAPTRACK_OK nothing changes, byte for byte (a frame whose pose was not
 *             accepted says nothing about the map).  Otherwise a landmark that is VISIBLE — stage 1 of "Tracking against the map", after
 *             the gates where there are any: a gated-out landmark is not visible — gets visible += 1; if it was KEPT by a keypoint in
 *             stage 3 and that keypoint's pair ended as an inlier after round 3, it also gets found += 1.  A landmark whose visible is
 *             INT32_MAX is not updated, so found <= visible always holds.  No atomics and no order dependence.  The recording costs one
 *             alignment kernel, one kernel over the call's rows and one more wait; with the switch off the three calls launch and wait
 *             for nothing new.
 *  Views      for landmark row s: n = the number of its views, the observation rows naming it, as in "Landmark refresh"; k_first = the kf
 *             of its first view in observation-table order that is a keyframe of the map (0 <= kf < nkf); age_kf = (nkf - 1) - k_first,
 *             or -1 without such a view.  If its keyframe was culled a landmark's first remaining view is later, so it looks younger:
 *             accepted.
 *  Rules      F (found ratio): found_ratio_pct > 0 and visible >= min_visible and (int64) found * 100 < (int64) found_ratio_pct * visible —
 *             strict, equality stays.  W (weak): weak_age_kf >= 0 and age_kf >= weak_age_kf and n <= weak_max_views; a landmark with
 *             age_kf == -1 is never weak.  A landmark is CULLED iff F or W holds, and counted at the FIRST that holds, F then W: reason 1
 *             for F, 2 for W.  culled_id comes out ascending.
 *  Apply      (apply != 0 and at least one landmark culled) dvs_backend_prune's cascade: the culled landmark rows and every observation
 *             row naming one leave both tables by ordered compaction, the other rows keep their order and every column; the statistics
 *             are compacted alongside; the keyframes' observation_ids lose the removed ids; keyframes stay even if emptied;
 *             observation_count and last_seen of the survivors are untouched, as are both id counters.  n_keyframes_touched = the
 *             keyframes whose observation_ids lost at least one id.  If nothing is culled, or apply == 0, the map stays byte for byte as it
 *             was and the three removal counts are 0.
 * DVS_ERR_ARG before any device work: found_ratio_pct > 100, min_visible < 1, weak_max_views < 0.  Count-then-capacity: *n_culled is always
 * set; DVS_ERR_CAPACITY, with nothing written and nothing applied, if an array is given and cap < *n_culled.  An empty map: DVS_OK, zeros.
 * The defaults — found_ratio_pct 25, min_visible 4, weak_age_kf 2, weak_max_views 1 — are usual values (ORB-SLAM's quarter and its two
 * keyframes), never fitted to a sensor.
 * Out of scope: a policy that calls the cull or switches recording on by itself, new landmark columns, decay or windowing of the counters,
 * counters merged on fusion, a class or id protection list, a scope argument, recording from dvs_maptrack_* calls made without a backend
 * or from relocalisation, creation of new landmarks, several GPUs. */
typedef struct dvs_lm_cull_params {
  int32_t found_ratio_pct;     /* 25; <= 0 switches rule F off; at most 100 */
  int32_t min_visible;         /* 4; >= 1 */
  int32_t weak_age_kf;         /* 2; < 0 switches rule W off */
  int32_t weak_max_views;      /* 1; >= 0 */
} dvs_lm_cull_params;          /* 16 bytes */
typedef struct dvs_lm_cull_result {
  int32_t n_landmarks;         /* rows examined */
  int32_t n_by_ratio, n_weak;  /* counted at the FIRST rule that holds: F, then W */
  int32_t n_landmarks_removed, n_observations_removed, n_keyframes_touched;   /* 0 with apply == 0 */
  int32_t reserved[2];
} dvs_lm_cull_result;          /* 32 bytes */
void dvs_lm_cull_default_params(dvs_lm_cull_params* p);
/* the recording switch, off in a new handle; allocates and launches nothing */
dvs_status dvs_backend_set_tracking_stats(dvs_backend* h, int32_t on);
/* out and the two arrays are nullable; each array takes *n_culled entries */
dvs_status dvs_backend_cull_landmarks(dvs_backend* h, const dvs_lm_cull_params* params /* NULL: defaults */, int32_t apply, dvs_lm_cull_result* out,
                                      int32_t cap, uint64_t* culled_id, int32_t* culled_reason, int32_t* n_culled);
/* The statistics and the views of every landmark row, rows as dvs_backend_get_landmarks; count-then-capacity (*n = landmark rows is always
 * set; DVS_ERR_CAPACITY, nothing written, if an array is given and cap < *n), every output nullable, the map never modified.
 * n_frames_recorded: the calls that recorded (status OK with the switch on) since the handle was created, reset or cleared. */
dvs_status dvs_backend_get_landmark_stats(dvs_backend* h, int32_t cap, uint64_t* id, int32_t* visible, int32_t* found, int32_t* n_views, int32_t* age_kf,
                                          int32_t* n, int64_t* n_frames_recorded);
/* What a caller that saves and reloads a map needs.  ids strictly ascending (else DVS_ERR_ARG, nothing changed); ids the map does not hold
 * are skipped; found > visible or a negative counter: DVS_ERR_ARG, nothing changed. */
dvs_status dvs_backend_set_landmark_stats(dvs_backend* h, int32_t n_rows, const uint64_t* id, const int32_t* visible, const int32_t* found);
/* all counters 0, n_frames_recorded 0; the switch stays as set */
dvs_status dvs_backend_clear_landmark_stats(dvs_backend* h);

/* ======================================= Relocalisation ================================= */
/* A frame's pose in the map WITHOUT a prior (csrc/reloc.hip; INTEGRATION.md "Relocalisation"): what recovers a tracker after a tracking
 * reset, when R_, t_ are stale and the window search of "Tracking against the map" finds nothing.  It is what ORB-SLAM's Relocalization
 * does after candidate selection (Mur-Artal, Montiel, Tardos 2015, section V-C: matches, PnP RANSAC, a guided search and a pose
 * optimisation that must keep enough inliers), as published ideas, with the candidate stage replaced by a search of the WHOLE landmark
 * table: one frame against a map is one Hamming contraction, which the matrix-core matcher runs with the landmarks as its query rows.
 * PARITY UNPINNED: the reference has no counterpart; the rule is the library's own, stated here in full and restated in numpy in
 * tests/reloc_ref.py.  Stages 1-3 are integers and are compared bit for bit; stage 4 is dvs_solve_pnp_ransac's procedure and is compared
 * byte for byte with that call; the host's Rodrigues conversion calls sin / cos and carries a tolerance.
 *  Inputs    n_lm landmarks — float xyz[3], uint8 desc[32], int64 id in ascending order (optional: a row index stands for the id) —,
 *            n_kp keypoints — dvs_keypoint, uint8 desc[32] —, the parameters.  No prior pose enters.
 *  Stage 1   global search, one landmark on its own, integers only.  Landmark row j with three finite coordinates is compared with every
 *            keypoint k < n_kp: d = hamming(desc_j, desc_k); best = the keypoint with the smallest (d, k); d_second = the smallest d among
 *            the OTHER keypoints (-1 if n_kp == 1).  The landmark PROPOSES to best iff d_best < max_hamming (strict) and (d_second < 0, or
 *            ratio_pct <= 0, or d_best * 100 < ratio_pct * d_second).  A landmark whose position is not finite is never compared and never
 *            proposes; with n_kp == 0 nothing is compared.
 *  Stage 2   one-to-one, as map tracking's stage 3.  Every keypoint KEEPS the proposal with the smallest (d, landmark row): one 64-bit
 *            integer minimum per proposal, so there is no tie deviation.  A landmark that loses stays unmatched.
 *  Stage 3   the list.  The kept pairs in ascending keypoint index, m of them: obj = the landmark's three floats, img = the keypoint's
 *            (x, y) floats.  m < min_pairs: status FEW_PAIRS, nothing is solved.
 *  Stage 4   pose from the list: dvs_solve_pnp_ransac's procedure, unchanged, on (obj, img, m, K4, pnp_iterations, pnp_reproj_err,
 *            pnp_confidence, seed), where the list lies.  One small record comes back: the call's first wait.  success == 0, or
 *            n_inliers < min_pnp_inliers, or an rvec / tvec that is not finite: status NO_POSE.  Otherwise the camera-to-world pose is
 *            formed on the host in FP64, every expression left to right as written: with w = rvec, th2 = (w0 w0 + w1 w1) + w2 w2,
 *            th = sqrt(th2), K = [w]x; th < 1e-12: R_cw = I + K; else A = sin(th) / th, B = (1 - cos(th)) / th2,
 *            R_cw[3i + j] = ((i == j) + A K[3i + j]) + B K2[3i + j], K2[3i + j] = (K[3i] K[j] + K[3i + 1] K[3 + j]) + K[3i + 2] K[6 + j];
 *            pnp_R = R_cw^T, pnp_t[i] = -((R_cw[i] * tvec0 + R_cw[3 + i] * tvec1) + R_cw[6 + i] * tvec2).
 *  Stage 5   confirmation: dvs_maptrack_track_device on the caller's dvs_maptrack handle with the same arrays and (pnp_R, pnp_t) as the
 *            prior; its record is embedded in the result.  Status OK iff track.status == DVS_MAPTRACK_OK and track.n_inliers >=
 *            min_confirmed, else NOT_CONFIRMED.
 *  Outcome   status 0 OK, 1 FEW_PAIRS, 2 NO_POSE, 3 NOT_CONFIRMED.  R, t = track.R, track.t with status 0, identity and zero otherwise;
 *            pnp_inliers, pnp_success, pnp_R, pnp_t and track are zeros with status 1 (and pnp_R, pnp_t, track with status 2).  Every status is DVS_OK.
 *            Two identical calls give identical bytes.
 * The defaults are usual values (ORB-SLAM's 50 / 0.75-style descriptor gates, OpenCV's 4 px and 0.99), never fitted to a sensor.
 * The handle owns a matcher context of its own, the top-2 arrays [n_lm][2], the per-keypoint keys and the list, all grow-only; it shares
 * nothing with the dvs_maptrack handle but the pose that crosses the host.  A program that never creates one allocates and launches
 * nothing it did not before.
 * Out of scope: candidate keyframes by votes or by the vocabulary, a depth-consistency gate on the pairs, a policy that calls it
 * automatically after a reset, octave and viewing-angle gates, several GPUs. */
typedef struct dvs_reloc dvs_reloc;
enum { DVS_RELOC_OK = 0, DVS_RELOC_FEW_PAIRS = 1, DVS_RELOC_NO_POSE = 2, DVS_RELOC_NOT_CONFIRMED = 3 };
typedef struct dvs_reloc_params {      /* 80 bytes */
  double K4[4];                        /* fx, fy, cx, cy: no default, zeros are refused (finite, fx, fy > 0) */
  int32_t max_hamming;                 /* 50; 0..257 */
  int32_t ratio_pct;                   /* 75; <= 0 switches the ratio test off; <= 100000 */
  int32_t min_pairs;                   /* 20; >= 4 */
  int32_t pnp_iterations;              /* 512; 1..1024 */
  double pnp_reproj_err;               /* 4.0 pixels; finite, > 0 */
  double pnp_confidence;               /* 0.99; inside (0, 1) */
  int32_t min_pnp_inliers;             /* 15; >= 0 */
  int32_t min_confirmed;               /* 30; >= 0 */
  uint64_t seed;                       /* 0: RANSAC's sampler seed */
} dvs_reloc_params;
typedef struct dvs_reloc_result {      /* 344 bytes */
  int32_t status;                      /* DVS_RELOC_* */
  int32_t n_proposed, n_pairs;         /* landmarks that proposed; kept pairs (m) */
  int32_t pnp_inliers, pnp_success;
  int32_t reserved;
  double pnp_R[9], pnp_t[3];           /* stage 4's pose, camera-to-world */
  dvs_maptrack_result track;           /* stage 5's record */
  double R[9], t[3];                   /* the confirmed pose with status 0, else identity and zero */
} dvs_reloc_result;
/* the defaults above; K4 stays zero */
void dvs_reloc_default_params(dvs_reloc_params* p);
/* DVS_ERR_ARG for parameters outside the ranges above, before any device work; then DVS_ERR_NO_DEVICE without a gfx950 (no CPU fallback).
 * The handle works on HIP's legacy default stream until dvs_reloc_set_stream.  Not thread-safe; buffers grow with the largest call. */
dvs_status dvs_reloc_create(const dvs_reloc_params* params, int32_t device, dvs_reloc** out);
void dvs_reloc_destroy(dvs_reloc* h);
dvs_status dvs_reloc_set_stream(dvs_reloc* h, void* hip_stream);   /* synchronises the old stream first */
/* Stages 1-5 on device arrays; mt confirms (same device; its image size and intrinsics are the caller's to make the frame's).  d_lm_id may
 * be NULL; descriptor arrays 16-byte aligned; n_lm * 2 and n_kp stay below 2^31.  Synchronises. */
dvs_status dvs_reloc_locate_device(dvs_reloc* h, dvs_maptrack* mt, const float* d_lm_xyz, const uint8_t* d_lm_desc, const int64_t* d_lm_id /* may be NULL */,
                                   int32_t n_lm, const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp, dvs_reloc_result* result);
/* the same with host pointers; a keypoint mt would not bin and ids that do not ascend strictly are DVS_ERR_ARG, as in dvs_maptrack_track */
dvs_status dvs_reloc_locate(dvs_reloc* h, dvs_maptrack* mt, const float* lm_xyz, const uint8_t* lm_desc, const int64_t* lm_id, int32_t n_lm,
                            const dvs_keypoint* kps, const uint8_t* desc, int32_t n_kp, dvs_reloc_result* result);
/* The last call's stage-3 list (each array nullable, count-then-capacity: *n = m is always set): the landmark row, the keypoint, the
 * distance and whether RANSAC ended with the pair as an inlier (all 0 with status 1). */
dvs_status dvs_reloc_get_pairs(dvs_reloc* h, int32_t cap, int32_t* lm_row, int32_t* kp_index, int32_t* dist, uint8_t* pnp_inlier, int32_t* n);
/* measurement (tools/reloc_timing.py; results are unaffected): with timing on, every locate call records four events on the handle's
 * stream — created by the first dvs_reloc_set_timing(h, 1), never otherwise — and ms3 = {stage 1, stages 2-3, stage 4 up to the export of
 * the record} of the last call; DVS_ERR_EMPTY without one. */
dvs_status dvs_reloc_set_timing(dvs_reloc* h, int32_t on);
dvs_status dvs_reloc_get_stage_ms(dvs_reloc* h, double* ms3);
/* dvs_reloc_locate_device with the backend's landmark table as it stands — position, descriptor and id columns handed over on the device;
 * the map is not modified.  Same device for the three handles; the backend's stream is synchronised first. */
dvs_status dvs_backend_relocalize_frame(dvs_backend* backend, dvs_reloc* h, dvs_maptrack* mt, const dvs_keypoint* d_kps, const uint8_t* d_desc, int32_t n_kp,
                                        dvs_reloc_result* result);
/* After a dvs_tracker_track: the last frame's depth-filtered keypoints and descriptors where the tracker left them in HBM, through
 * dvs_backend_relocalize_frame.  With apply != 0 and status 0, R, t replace R_, t_, so the next frame's odometry composes on them, as
 * dvs_tracker_track_map does.  DVS_ERR_EMPTY before the first frame; after a frame with tracking_reset the set may be empty, which is
 * status FEW_PAIRS, not an error.  Strictly opt-in: nothing calls it after a reset but the caller. */
dvs_status dvs_tracker_relocalize(dvs_tracker* tracker, dvs_backend* backend, dvs_reloc* h, dvs_maptrack* mt, int32_t apply, dvs_reloc_result* result);

#ifdef __cplusplus
}
#endif
#endif /* DVSLAM_HIP_H */
