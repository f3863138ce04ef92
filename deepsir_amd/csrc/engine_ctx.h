// What the host-side translation units of libdsir.so share: the context, its workspace, the scope of one C-ABI call (Call), the weight
// tables and the functions that cross files.  engine.hip: life cycle, tuning gate, switches; register.hip: the registration and
// forward_pair; entries_stage.hip / entries_pose.hip: the stage and pose entries; weights.hip: expected keys and uploads;
// schedule.hip: the layer schedule of RandLA.forward / aggregation and the KNN pyramid; search.hip: the descriptor search.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "dsir.h"
#include "kernels.h"
#include "search_plan.h"

namespace dsir {

// ------------------------------------------------------------------ parameters
struct HostParam {
  std::string name;
  std::vector<int64_t> shape;
  std::vector<float> data;
  bool loaded = false;
  bool ignored = false;  // num_batches_tracked
  int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};

struct Mlp2dW { const float *W = nullptr, *b = nullptr, *gamma = nullptr, *beta = nullptr; int cin = 0, cout = 0, groups = 0; };
struct AttW { const float* fc = nullptr; const float* fc_g = nullptr; int d = 0; Mlp2dW mlp; };   // fc_g: see up_fc_g
struct BlockW { Mlp2dW mlp1, lfa1, lfa2, mlp2, skip; AttW att1, att2; int d_in = 0, d = 0; const float* lse_w8 = nullptr;   // lse_w8: up_lse_uv
                const float *pair_W = nullptr, *pair_b = nullptr; };   // mlp1's rows followed by mlp_skip's (and the biases likewise): up_pair
struct LinW { const float *W = nullptr, *b = nullptr; int cin = 0, cout = 0; };
struct RandlaW { Mlp2dW pre; BlockW blk[4]; Mlp2dW mid; Mlp2dW dec[4]; const float* out_w = nullptr; int dec_out = 0; LinW fc[3]; int cin = 0, ncls = 0;
                 bool ppf = false;   // DSIR_FLAG_PPF: mlp_pre is the point-pair-feature layer (ppf.hip), level 0 takes 12 channels
                 const void* head_wh[4] = {}; const void* head_wl[4] = {}; };   // fp16 split of mlp_out + fc_label (head_mlp.hip)
struct NetW { RandlaW feat, inl; LinW mlp_feat[3], mlp_att[5], mlp_proj; };

// ------------------------------------------------------------------ workspace
struct Arena {
  char* base = nullptr;
  size_t cap = 0, top = 0;
  bool overflow = false;
  void* raw(size_t bytes) {
    size_t a = (top + 255) & ~(size_t)255;
    if (a + bytes > cap) { overflow = true; return base; }
    top = a + bytes;
    return base + a;
  }
  template <typename T> T* get(size_t count) { return reinterpret_cast<T*>(raw(count * sizeof(T))); }
  size_t mark() const { return top; }
  void release(size_t m) { top = m; }
};

struct Pyramid {     // KNN pyramid of a cloud batch, levels concatenated (data_base.py:178-181)
  int clouds = 0, n = 0;
  int nl[DSIR_MAX_LEVELS + 1] = {};
  int off[DSIR_MAX_LEVELS + 1] = {};   // level offsets into xyz / neigh / interp
  int soff[DSIR_MAX_LEVELS + 1] = {};  // level offsets into sub
  int S = 0, S1 = 0;
  const float* xyz = nullptr;     // [clouds][S][3]
  const int32_t* neigh = nullptr; // [clouds][S][16]
  const int32_t* sub = nullptr;   // [clouds][S1][16]
  const int32_t* interp = nullptr;// [clouds][S]
};

// What is meaningful within ONE C-ABI call only: opening a call (Call, below) assigns CallState{} and rewinds the arena with it
struct CallState {
  const char* sched_error = nullptr;   // a launcher refused a layer (outside its envelope): reported by Call::finish / overflow_fail
  size_t stats_top = 0;                // GroupNorm statistics slots handed out to the running pass
  size_t stats_base = 0;               // dsir_register: the passes of one call take consecutive regions of an arena zeroed ONCE
  bool stats_prezeroed = false;
  int walk_used = 0;                   // walker programs of this call
  bool walk_begun = false;             // this call took a pinned staging set (Call::begin_walker): its event is owed
};

// a tensor with a lazily applied GroupNorm (+activation)
struct Act {
  float* p = nullptr;
  int C = 0;
  int rows = 0;       // rows per cloud
  GnRef gn = {nullptr, nullptr, nullptr, 0, 0.0};
  int act = 0;
  // lse_uv.hip: the position-encoding layer of levels 0 / 1 is not in memory (p == nullptr): per-point tables instead
  const float* uv = nullptr;      // [clouds][rows / 16][2 C]
  const float* dist = nullptr;    // [clouds][rows]
  const float* w8 = nullptr;
};

}  // namespace dsir

struct dsir_ctx {
  int device = 0;
  dsir_cfg cfg{};
  int flags = 0;                       // DSIR_FLAG_* of dsir_create_ex
  hipStream_t stream = nullptr;        // where every launch of this context goes: own_stream, or a caller's (dsir_set_stream)
  hipStream_t own_stream = nullptr;
  std::string err;
  dsir::CallState call;                // reset, together with ws.top / ws.overflow, by every call's opening
  std::vector<dsir::HostParam> params;
  std::unordered_map<std::string, int> index;
  float* dweights = nullptr;
  uint16_t* dweights16 = nullptr;        // fp16 split of the WHOLE weight blob: high parts [0, n), low parts [n, 2 n), same offsets
  size_t nweights = 0;                   // floats in dweights
  const void* agg_wh[5] = {}; const void* agg_wl[5] = {};   // unset when one of the five is outside the split's domain
  // Matrices of the blob outside the split's domain (split_f16.h), as [first, end) offsets in load order: their layers run
  // in exact fp32.  Empty for weights of ordinary magnitudes.
  std::vector<std::pair<size_t, size_t>> split_off;
  bool split_ok(size_t off) const {
    for (const auto& r : split_off)
      if (off >= r.first && off < r.second) return false;
    return true;
  }
  bool finalized = false;
  dsir::NetW net;
  dsir::Arena ws;
  double* stats = nullptr;   // GroupNorm statistics slots
  size_t stats_cap = 0;
  // nn_match timing
  bool time_match = false;
  // hipGraph replay of dsir_register (launch-bound small batches)
  bool use_graph = false;
  // captured registrations, one per distinct call signature (sizes AND buffer addresses): a server that batches 1 .. K
  // single-pair requests into one call replays K graphs in turn (deepsir_amd/serve.py); the oldest is evicted beyond kMaxGraphs
  struct Graph { std::vector<unsigned char> key; hipGraphExec_t exec; void* walk_block; };   // walk_block: the graph's walker programs (device)
  int64_t graph_nodes[4] = {0, 0, 0, 0};   // the latest captured registration: nodes in all, kernel / memset / memcpy nodes (dsir_graph_stats)
  // ---- deep-level walker (walk.hip): the programs of one call's RandLA passes live in device memory
  static constexpr int kWalkSlots = 12;        // programs per call (1 extractor pass or 2, up to 10 inlier passes)
  static constexpr int kWalkClouds = 16;       // the walker serves launches of up to that many clouds
  int walk_mode = 0;                           // 1: the deep levels of a pass as one launch (dsir_enable_walk / DSIR_WALK=1); OFF by default -
                                               // measured slower than the launches it replaces (walk.hip, "What it measured")
  dsir::WalkProgram* walk_dev = nullptr;             // eager calls: device programs, filled by in-stream copies from ...
  dsir::WalkProgram* walk_host[2] = {nullptr, nullptr};   // ... pinned staging, two sets taken in turn by consecutive calls
  hipEvent_t walk_ev[2] = {nullptr, nullptr};  // recorded after a call's last copy from the set
  bool walk_ev_armed[2] = {false, false};
  int walk_set = 0;
  unsigned* walk_ctr = nullptr;                // [kWalkSlots][kWalkClouds][kWalkCtrWords] tile queues / completion counters
  unsigned long long* walk_trace = nullptr;    // measurement (DSIR_WALK_TRACE, dsir_walk_trace): [kWalkSlots][kWalkMaxPhases][4] device-clock stamps
  int walk_wpc = 0;                            // tuning hook (DSIR_WALK_WPC): workgroups per cloud, 0 = by launch size
  int walk_flags = 0;                          // tuning hook (DSIR_WALK_FLAGS): WalkProgram::flags
  // a registration under capture: programs are collected on the host and uploaded ONCE, after the capture, into the graph's own block
  bool capturing = false;
  std::vector<unsigned char> cap_host;
  dsir::WalkProgram* cap_dev = nullptr;
  std::vector<Graph> graphs;
  static constexpr size_t kMaxGraphs = 16;
  void drop_graphs() {
    for (auto& g : graphs) { hipGraphExecDestroy(g.exec); if (g.walk_block) hipFree(g.walk_block); }
    graphs.clear();
  }
  struct MatchEvents { hipEvent_t op0, op1, k0, k1; };   // whole operation / its dominant kernel alone
  std::vector<MatchEvents> match_events;
  size_t match_events_used = 0;
  double match_ms = 0.0, match_kernel_ms = 0.0;
  int64_t match_launches = 0;
  // arg-min path of dsir_register: 1 = screened (nn_screen.hip) for large problems, 0 = always the exhaustive kernel
  int screen_mode = 1;
  int prune_min_points = 8192;          // pruned search (nn_prune.hip) for ref clouds of that many points and more; 0 = off
  long long prune_min_rows = 65536;     // ... in launches of that many src rows (pairs x points) and more
  // aggregation chain: 1 = fp16-split products on the fp16 matrix pipe, 0 = exact-fp32 chain (agg_chain.hip)
  int agg_split = 1;
  int kabsch_chunked_min = 0;           // clouds of that many points and more solve their pose in chunks; 0 = kKabschChunkedMin
  // device-clock brackets {first wave start, last wave end} of the timed nn_match launches
  unsigned long long* match_ts = nullptr;    // [kMatchSlots][2]
  size_t match_ts_used = 0;
  double match_dev_ms = 0.0;
  int64_t match_dev_launches = 0;
  // running totals of the screened arg-min inside dsir_register (dsir_screen_stats)
  unsigned long long* screen_acc = nullptr;   // device, 4 x u64 (+ 2 x u64: tile products kept / in all by the pruned search)
  int64_t exhaustive_searches = 0;            // searches that took the exhaustive kernel directly (small problems)
};

namespace dsir {

int fail(dsir_ctx* c, const char* fmt, ...);     // c == nullptr: the creation error of this thread (dsir_last_error(NULL))

#define HIP_OK(c, expr)                                                                 \
  do {                                                                                  \
    hipError_t e__ = (expr);                                                            \
    if (e__ != hipSuccess) return fail((c), "%s: %s", #expr, hipGetErrorString(e__));   \
  } while (0)

// ws.overflow is set: report the launcher's refusal that stopped the schedule (Sched::refuse), else the arena's exhaustion
inline int overflow_fail(dsir_ctx* c, const char* exhausted) { return fail(c, "%s", c->call.sched_error ? c->call.sched_error : exhausted); }

static_assert(kMaxLevels == DSIR_MAX_LEVELS, "kernels.h and dsir.h disagree on the level count");

// the workspace is sized from max_pairs and max_points: inside them no allocation of a call can overflow
inline int check_batch(dsir_ctx* c, const char* name, int clouds, int n) {
  if (clouds > 2 * c->cfg.max_pairs || n > c->cfg.max_points) return fail(c, "%s: batch exceeds max_pairs/max_points", name);
  return 0;
}

// The scope of one C-ABI call on a context.  Every entry that enqueues work opens one first - null context, weights (kWeights),
// hipSetDevice, then the arena rewound and the call state reset - and leaves through finish().  An error return in between leaves
// through the destructor: it still covers the walker's staging copies with their event and clears the call state; it makes no
// other HIP call, never synchronises and never touches c->err.
class Call {
 public:
  enum Needs { kContext, kWeights };
  explicit Call(dsir_ctx* c, Needs needs = kContext) : c_(open(c, needs) ? nullptr : c) {}
  ~Call() { if (c_) { end_walker(c_); reset(c_); } }
  bool refused() const { return !c_; }
  int begin_walker();     // schedule.hip: before the first RandLA pass of a call
  int finish() {
    dsir_ctx* c = c_;
    c_ = nullptr;         // the call state stays readable until the next opening
    if (hipError_t e = end_walker(c)) return fail(c, "hipEventRecord(c->walk_ev[c->walk_set], c->stream): %s", hipGetErrorString(e));
    if (c->ws.overflow) return overflow_fail(c, "workspace exhausted (raise max_points / max_pairs in dsir_cfg)");
    if (hipError_t e = hipGetLastError()) return fail(c, "HIP launch error: %s", hipGetErrorString(e));
    return 0;
  }

 private:
  dsir_ctx* c_;
  static void reset(dsir_ctx* c) { c->ws.top = 0; c->ws.overflow = false; c->call = CallState{}; }
  static int open(dsir_ctx* c, Needs needs) {
    if (!c) return 1;
    if (needs == kWeights && !c->finalized) return fail(c, "weights not finalized (call dsir_load_weight for every key, then dsir_finalize_weights)");
    HIP_OK(c, hipSetDevice(c->device));
    reset(c);
    return 0;
  }
  static hipError_t end_walker(dsir_ctx* c);     // schedule.hip
};

// ------------------------------------------------------------------ GroupNorm statistics regions
// Every RandLA pass takes one region of the statistics arena; the passes of a registration take consecutive regions of an arena zeroed
// once (register_enqueue).  A pass has 34 GroupNorm layers (35 under use_ppf); its region is sized for kGnLayersPerPass of them.
constexpr int kGnLayersPerPass = 40;
// words one GroupNorm layer's statistics take for `clouds` clouds
inline size_t gn_layer_words(size_t clouds, int groups = 8) { return clouds * groups * kGnWords; }
inline size_t gn_pass_words(size_t clouds) { return (size_t)kGnLayersPerPass * gn_layer_words(clouds); }
// a registration's passes side by side: the feature extractor on 2 P clouds, n_iter inlier passes on P
inline size_t gn_register_words(int P, int n_iter) { return gn_pass_words((size_t)2 * P + (size_t)n_iter * P); }

// ------------------------------------------------------------------ schedule.hip
inline Seg plain_seg(const float* x, int64_t cloud_stride, int C, int ld, const int32_t* idx = nullptr, int64_t idx_cs = 0) {
  Seg s{};
  s.x = x; s.cloud_stride = cloud_stride; s.C = C; s.ld = ld; s.idx = idx; s.idx_cloud_stride = idx_cs;
  s.gn = GnRef{nullptr, nullptr, nullptr, 0, 0.0}; s.act = 0;
  return s;
}

// The position-encoding branch of every level (lfa.mlp1 on the relative position code, lfa.mlp2 on top of it)
// depends only on the pyramid and the weights.  The inlier model runs on the SAME (src) pyramid in every
// registration iteration (model.py:575), so that branch is computed in iteration 0 into caller-owned
// storage and re-used afterwards: same kernels, same inputs, same bits (SURVEY §7.2 loop invariants).
struct EncCache {
  bool valid = false;
  float* s2_buf[DSIR_MAX_LEVELS][2] = {};   // enc half of the attention scores (W2 enc / W2 enc2) of the levels that keep them (att_keeps_score_cache)
  float* enc_buf[DSIR_MAX_LEVELS] = {};
  float* uv_buf[DSIR_MAX_LEVELS] = {};     // levels whose lfa.mlp1 rows are not stored (lse_uv.hip): tables + dist instead of enc_buf
  float* dist_buf[DSIR_MAX_LEVELS] = {};
  float* enc2_buf[DSIR_MAX_LEVELS] = {};
  double* enc_stats[DSIR_MAX_LEVELS] = {};
  double* enc2_stats[DSIR_MAX_LEVELS] = {};
  Act enc[DSIR_MAX_LEVELS], enc2[DSIR_MAX_LEVELS];
  // statistics words of the cache for P clouds: two layers per level
  static size_t stats_words(const dsir_cfg& g, int P) { return (size_t)2 * g.num_layers * gn_layer_words(P); }
  // persistent storage of the inlier model's branch on the pyramid `ps`, alive across the iterations, from the context's arena.
  // prezeroed: stats_words() words zeroed by the registration's opening launch, or nullptr (own storage, own memset)
  int plan(dsir_ctx* c, const Pyramid& ps, double* prezeroed);
};

// what the descriptor search needs of the descriptors besides their values (AggArgs: sq, hi / lo, packed_init); the fp16-split chain
// writes them in its epilogue and returns true, any other path leaves them to the search's own preparation kernels
struct AggExtras { float* sq = nullptr; void* hi = nullptr; void* lo = nullptr; unsigned long long* packed_init = nullptr; };

void fill_pyramid_layout(const dsir_cfg& cfg, int clouds, int n, Pyramid& p);
int gn_max_contributions(const dsir_cfg& g, int n, int flags = 0);
int randla_forward(dsir_ctx* c, const RandlaW& w, const Seg& in0, const Seg* in1, const Pyramid& py, float* feat_out,
                   float* logits_out, EncCache* cache = nullptr);
int run_lfa_enc2_probe(dsir_ctx* c, const RandlaW& w, int level, int fused, const Pyramid& py, float* rows_out, double* stats_out);
int run_ppf_pre(dsir_ctx* c, const RandlaW& w, const float* rows, int stride, const int32_t* neigh, int64_t neigh_cs, int clouds, int n,
                float* out);
// How mlp_feat is launched.  Auto: the fused launch (feat_chain.hip) where it takes the layers and the launch is large enough
// (feat_chain_wanted, schedule.hip), else the three launches.  Three: the three launches.  Fused: the fused launch or nothing
// (nullptr returned: refused).  max_blocks > 0 caps the fused launch's grid (the probe's way to several tiles per wave).
enum class FeatForm { Auto, Three, Fused };
// mlp_feat.  out: caller-owned [clouds][n][64] or the arena.
float* run_mlp_feat(dsir_ctx* c, const float* feat0, int clouds, int n, float* out = nullptr, FeatForm form = FeatForm::Auto, int max_blocks = 0);
// both sides of a registration, feat0 = [2 P][n][64]: the first P clouds into out_a (caller-owned), the others into the arena
// (returned) - one launch where the fused form runs, else side by side as run_mlp_feat does them
float* run_mlp_feat_pair(dsir_ctx* c, const float* feat0, int P, int n, float* out_a, FeatForm form = FeatForm::Auto, int max_blocks = 0);
int run_mlp_feat_probe(dsir_ctx* c, const float* feat0, int clouds, int n, int fused, int max_blocks, float* out);
bool run_att_proj(dsir_ctx* c, const float* xyz, int64_t xyz_cs, const float* score, const float* F, int clouds, int n,
                  float* desc, const AggExtras* ex = nullptr);
int build_pyramid(dsir_ctx* c, const float* points, int stride, int clouds, int n, float* xyz, int32_t* neigh,
                  int32_t* sub, int32_t* interp);

// ------------------------------------------------------------------ weights.hip
void expect_state_dict(dsir_ctx* c);     // the keys and shapes dsir_load_weight accepts (mirrors deepsir_amd/arch.py)

// ------------------------------------------------------------------ search.hip
// The descriptor search of a registration and of the stand-alone entry points (dsir_nn_match, dsir_nn_match_screened,
// dsir_screen_bounds): nearest ref descriptor of every src descriptor, in the mode search_plan.h chose.
struct DescSearch {
  dsir_ctx* c;
  SearchMode mode;
  int P, J, K;
  bool timed = false;      // bracket the operation with the context's match events (dsir_enable_match_timer)
  bool counted = false;    // a registration's search: the context's running totals and device-clock slots
  void* match_scratch = nullptr;                      // exhaustive kernel: norms + packed result slots
  void *ah = nullptr, *al = nullptr, *bh = nullptr, *bl = nullptr;   // screened: fp16 operand pairs of src (a) and ref (b)
  float *sa = nullptr, *sb = nullptr;                 // ... and the rows' squared norms
  void* scratch = nullptr;                            // ... and the candidate scratch
  void* prune_scratch = nullptr;
  unsigned long long* stats = nullptr;                // optional {rows, rows left to the exhaustive kernel} of one search
  int32_t* bad = nullptr;                             // optional flag: an element outside the screening's domain
  AggExtras ex_ref, ex_src;
  const int32_t* prev_idx = nullptr;                  // the previous run's matches (pruned search: every row's first upper bound)
  // every operand and scratch region from the context's arena (the caller checks ws.overflow).  match_scratch: also for the
  // screened modes (a registration keeps it for pairs the screening hands back)
  void alloc(bool with_match_scratch, bool with_stats = false, bool with_bad = false);
  // what the aggregation epilogue should leave for the search (run_att_proj), nullptr: nothing
  const AggExtras* ref_extras() const { return search_screens(mode) ? &ex_ref : nullptr; }
  const AggExtras* src_extras() const { return mode == SearchMode::forced ? nullptr : &ex_src; }
  // stand-alone calls own both sides: clear the domain flag, split and norm src, then ref
  int split_pair(const float* a, const float* b);
  // ref side, once: split and norm unless the aggregation epilogue did (prepared), then the pruned search's column order
  int prepare_ref(const float* desc_r, bool prepared, const float* rxyz, int64_t rxyz_cs);
  struct Iter {
    int it = 0;                            // iteration of the registration: later ones keep the gate / the cached ref norms
    bool src_prepared = false;             // the src operands are in place (aggregation epilogue, split_pair)
    const int32_t* forced = nullptr;       // forced: the caller's correspondences of this iteration ...
    int32_t* invalid = nullptr;            // ... and the pairs' flags for out-of-range entries
    bool domain_gate = false;              // hand `bad` to the screening: out-of-domain inputs take the exhaustive kernel
    bool want_stats = false;               // fill `stats`
  };
  int run(const float* desc_s, const float* desc_r, int32_t* idx_out, const Iter& i);
  // the k nearest per row with distances (nn_topk.hip), exhaustive mode only: bytes alloc_topk takes from the arena, the
  // allocation (the caller checks ws.overflow, or compares topk_bytes against the arena first), the run
  void* topk_scratch = nullptr;
  size_t topk_bytes(int k) const { return nn_topk_scratch_bytes(P, J, K, k); }
  void alloc_topk(int k) { topk_scratch = c->ws.raw(topk_bytes(k)); }
  int run_topk(const float* desc_s, const float* desc_r, int k, int32_t* idx_out, float* dist_out);
};
constexpr size_t kMatchSlots = 4096;

}  // namespace dsir
