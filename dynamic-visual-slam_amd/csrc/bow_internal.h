// bow_internal.h — what bow.hip (transform, database), bow_train.hip (vocabulary training) and loop.hip (direct index, guided matching)
// share: the vocabulary's device view, its host form, the two handles, the three entry points of bow.hip that training builds on and the
// inverted part of a database that loop.hip builds on.  Internal to the library; nothing here is exported.
#pragma once
#include <vector>
#include "common.h"
#include "device_mem.h"

namespace dvs {

struct VocabDev {
  const uint4* desc;        // [nodes][2]: 32-byte rows, children of one node contiguous in child-list order
  const int* child_begin;   // first child's row
  const int* child_count;
  const int* word_id;       // -1 for inner nodes
  const int* orig_id;       // the node id callers see
  const double* weight;
};

struct HostVocab {
  int k = 0, L = 0, scoring = 0, weighting = 0, n_nodes = 0, n_words = 0;
  std::vector<uint8_t> desc;   // rows in device order (row 0: the root, zeros)
  std::vector<int> child_begin, child_count, word_id, orig_id;
  std::vector<double> weight;
};

// bow.hip: header and tree checks, then the breadth-first rows (no device work)
dvs_status bow_build_vocab(int k, int L, int scoring, int weighting, int n, const int32_t* parent, const uint8_t* is_leaf, const uint8_t* desc,
                           const double* weight, HostVocab* H);
// bow.hip: the handle of a checked vocabulary (uploads its rows)
dvs_status bow_create_vocab(int device, void* hip_stream, const HostVocab& H, dvs_bow_vocab** out);
// bow.hip: k_bow_descend alone, enqueued on `s`: every feature's word, node and weight (blocks of [nframes][stride_rows])
dvs_status bow_enqueue_descend(const VocabDev& V, const uint8_t* d_desc, const int* d_n, int stride_rows, int nframes, int nid_level, int* feat_word,
                               int* feat_node, double* feat_weight, hipStream_t s);

// a block that grows and keeps its contents (the copy is ordered on `s`, which is drained before the old block is freed)
template <class T>
dvs_status grow_keep(DeviceBuf<T>& buf, size_t& cap, size_t need, size_t used, hipStream_t s) {
  if (need <= cap) return DVS_OK;
  DeviceBuf<T> bigger;
  const size_t ncap = need + need / 2;
  DVS_TRY(bigger.alloc(ncap));
  if (used) DVS_HIP(hipMemcpyAsync(bigger.get(), buf.get(), used * sizeof(T), hipMemcpyDeviceToDevice, s));
  DVS_HIP(hipStreamSynchronize(s));
  buf = std::move(bigger);
  cap = ncap;
  return DVS_OK;
}

}  // namespace dvs

struct dvs_bow_vocab {
  int device = 0;
  hipStream_t stream = nullptr;
  dvs::HostVocab H;            // the sizes; its arrays are released after the upload
  dvs::DeviceBuf<uint8_t> desc;
  dvs::DeviceBuf<int> child_begin, child_count, word_id, orig_id;
  dvs::DeviceBuf<double> weight;
  dvs::VocabDev V{};
  // scratch and the handle's own outputs, [frames][rows] ([frames][rows + 1] for the two offset blocks), grown on demand
  size_t cap_rows = 0, cap_frames = 0, cap_in = 0;
  dvs::DeviceBuf<int> sw_word, sw_feat, sn_node, seg_start;
  dvs::DeviceBuf<int> o_word_ids, o_fv_nodes, o_fv_offsets, o_fv_features, o_feat_word, o_feat_node, o_n_words, o_n_fv;
  dvs::DeviceBuf<double> o_word_values, o_feat_weight;
  dvs::DeviceBuf<uint8_t> in_desc;  // the host forms' staging: one frame's rows and its count
  dvs::DeviceBuf<int> in_n;
  dvs::PinnedBuf<int> h_n;
};

// the inverted part of a keyframe database: dvs_bow_db is exactly this, dvs_loop_db (loop.hip) embeds one
struct dvs_bow_db {
  dvs_bow_vocab* voc = nullptr;
  int n_entries = 0;
  long long nnz_bound = 0;     // no fewer than the words stored (device frames are counted by their rows until the count is read back)
  size_t cap_off = 0, cap_nnz_w = 0, cap_nnz_v = 0, cap_raw = 0, cap_common = 0, cap_ids = 0, cap_scores = 0;
  dvs::DeviceBuf<long long> off;
  dvs::DeviceBuf<int> words, common, ids, counters;   // counters: [0] entries with a common word, [1] results
  dvs::DeviceBuf<double> values, raw, scores;
};

namespace dvs {

// bow.hip, the ONE implementation of the inverted part.  A frame is transformed once, into the vocabulary's own blocks (o_*, frame f at
// f * stride_rows, offsets at f * (stride_rows + 1)), at the `levelsup` the caller's FeatureVector wants (the BowVector does not depend
// on it); what follows reads those blocks, which stay valid until the handle's next transform.
dvs_status bow_db_init(dvs_bow_db* db, dvs_bow_vocab* voc);                 // the blocks an empty database needs
dvs_status bow_stage_frame(dvs_bow_vocab* v, const uint8_t* desc, int n);   // one host frame into in_desc / in_n (asynchronous)
dvs_status bow_transform_own(dvs_bow_vocab* v, const uint8_t* d_desc, const int* d_n, int stride_rows, int nframes, int levelsup);
int bow_query_limit(const dvs_bow_db* db, int max_results, int max_id);     // the most results a query can give
// frame 0 of the own blocks against the entries: ids / scores / count to device memory (capacity bow_query_limit)
dvs_status bow_db_query_own(dvs_bow_db* db, int stride_rows, int max_results, int max_id, int* d_ids, double* d_scores, int* d_n_results);
// scratch, reserve, transform at `levelsup`, append: the frames become entries n_entries ... (what dvs_bow_db_add[_device] run)
dvs_status bow_db_add_device(dvs_bow_db* db, const uint8_t* d_desc, const int* d_n, int stride_rows, int nframes, int levelsup);
// dvs_bow_db_query after its argument checks; `what` names the caller in messages
dvs_status bow_db_query_host(dvs_bow_db* db, const uint8_t* desc, int n, int max_results, int max_id, int levelsup, int* ids, double* scores, int cap,
                             int* n_results, const char* what);

}  // namespace dvs
