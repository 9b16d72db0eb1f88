// bow_internal.h — what bow.hip (transform, database) and bow_train.hip (vocabulary training) share: the vocabulary's device view, its
// host form, the handle, and the three entry points of bow.hip that training builds on.  Internal to the library; nothing here is exported.
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
