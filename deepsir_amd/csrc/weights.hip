// The weights of libdsir.so: the state-dict keys a context expects (mirrors deepsir_amd/arch.py), their folding and upload into one
// device blob (plus its fp16 split), and the tables the schedule reads (NetW).
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "engine_ctx.h"

namespace dsir {

namespace {

// ------------------------------------------------------------------ expected state-dict (mirrors deepsir_amd/arch.py)
void add_param(dsir_ctx* c, const std::string& name, std::vector<int64_t> shape, bool ignored = false) {
  HostParam p;
  p.name = name; p.shape = std::move(shape); p.ignored = ignored;
  c->index[name] = (int)c->params.size();
  c->params.push_back(std::move(p));
}
void add_mlp2d(dsir_ctx* c, const std::string& pre, int cin, int cout) {
  add_param(c, pre + ".conv.weight", {cout, cin, 1, 1});
  add_param(c, pre + ".conv.bias", {cout});
  add_param(c, pre + ".norm.weight", {cout});
  add_param(c, pre + ".norm.bias", {cout});
}
void add_att(dsir_ctx* c, const std::string& pre, int din, int dout) {
  add_param(c, pre + ".fc.weight", {din, din, 1, 1});
  add_mlp2d(c, pre + ".mlp", din, dout);
}
void add_mlp1d(dsir_ctx* c, const std::string& pre, const std::vector<int>& ch) {
  int pos = 0;
  const int n = (int)ch.size();
  for (int i = 1; i < n; ++i) {
    const std::string p = pre + "." + std::to_string(pos);
    add_param(c, p + ".weight", {ch[i], ch[i - 1], 1});
    add_param(c, p + ".bias", {ch[i]});
    ++pos;
    if (i < n - 1) {
      const std::string q = pre + "." + std::to_string(pos);
      add_param(c, q + ".weight", {ch[i]});
      add_param(c, q + ".bias", {ch[i]});
      add_param(c, q + ".running_mean", {ch[i]});
      add_param(c, q + ".running_var", {ch[i]});
      add_param(c, q + ".num_batches_tracked", {}, true);
      pos += 2;
    }
  }
}
void add_randla(dsir_ctx* c, const std::string& pre, int cin, int ncls) {
  const dsir_cfg& g = c->cfg;
  const bool ppf = (c->flags & DSIR_FLAG_PPF) != 0;       // RandLANet.py:251-254: d_feat_in = 10, dim_temp = 12
  int dim = ppf ? 12 : 8;
  add_mlp2d(c, pre + ".mlp_pre", ppf ? 10 : cin, dim);
  for (int i = 0; i < g.num_layers; ++i) {
    const int d = g.d_out[i];
    const std::string p = pre + ".dilated_res_blocks." + std::to_string(i);
    add_mlp2d(c, p + ".mlp1", dim, d / 2);
    add_mlp2d(c, p + ".lfa.mlp1", 10, d / 2);
    add_att(c, p + ".lfa.att_pooling_1", d, d / 2);
    add_mlp2d(c, p + ".lfa.mlp2", d / 2, d / 2);
    add_att(c, p + ".lfa.att_pooling_2", d, d);
    add_mlp2d(c, p + ".mlp2", d, 2 * d);
    add_mlp2d(c, p + ".mlp_skip", dim, 2 * d);
    dim = 2 * d;
  }
  add_mlp2d(c, pre + ".mlp_mid", dim, dim);
  int dcur = dim;
  const int L = g.num_layers;
  for (int j = 0; j < L; ++j) {
    int cin_j;
    if (j < L - 1) { cin_j = dcur + 2 * g.d_out[L - j - 2]; dcur = 2 * g.d_out[L - j - 2]; }
    else { cin_j = 4 * g.d_out[0]; dcur = 2 * g.d_out[0]; }
    add_mlp2d(c, pre + ".decoder_blocks." + std::to_string(j), cin_j, dcur);
  }
  add_param(c, pre + ".mlp_out.weight", {g.out_feat_dim, dcur, 1, 1});
  add_mlp1d(c, pre + ".fc_label", {g.out_feat_dim, 64, 32, ncls});
}

}  // namespace

void expect_state_dict(dsir_ctx* c) {
  const dsir_cfg* cfg = &c->cfg;
  // which sub-networks exist follows args.pipeline (model.py:131-193)
  add_randla(c, "feat_extractor", cfg->feat_len, cfg->num_classes);
  if (cfg->pipeline != DSIR_PIPELINE_LABEL) {
    add_mlp1d(c, "mlp_feat", {64, 64, 128, 64});
    add_mlp1d(c, "mlp_att", {4, 32, 64, 128, 256, 64});
    add_mlp1d(c, "mlp_proj", {64, 64});
  }
  if (cfg->pipeline == DSIR_PIPELINE_ALIGN) add_randla(c, "inlier_model", 6, 1);
}

namespace {

// ------------------------------------------------------------------ weight upload
struct Uploader {
  std::vector<float> blob;
  std::vector<std::pair<size_t, size_t>> spans;      // [first, end) of every array, in upload order
  size_t put(const std::vector<float>& v) {
    size_t o = (blob.size() + 63) & ~(size_t)63;
    blob.resize(o + v.size());
    std::memcpy(blob.data() + o, v.data(), v.size() * sizeof(float));
    spans.emplace_back(o, o + v.size());
    return o;
  }
};

// Is a matrix inside the domain of the fp16 split (split_f16.h)?  Every entry within the fp16 range, and the two parts
// together carrying the matrix to 2^-19 of its Frobenius norm: sum (w - hi - lo)^2 <= 2^-38 sum w^2.  Entries whose low part
// is sub-normal (|w| < 2^-3) lose up to 2^-25 each, whatever their size; He-normal matrices of 10..768 inputs sit at 2^-22,
// the same matrix times 2^-6 at 2^-16.
bool split_in_domain(const float* w, const uint16_t* hi, const uint16_t* lo, size_t n) {
  double r2 = 0.0, f2 = 0.0;
  for (size_t i = 0; i < n; ++i) {
    if (!(std::fabs(w[i]) <= 65504.f)) return false;
    _Float16 h, l;
    std::memcpy(&h, hi + i, 2); std::memcpy(&l, lo + i, 2);
    const double r = (double)w[i] - (double)(float)h - (double)(float)l;
    r2 += r * r; f2 += (double)w[i] * (double)w[i];
  }
  return r2 <= 0x1p-38 * f2;
}

const HostParam& P(dsir_ctx* c, const std::string& name) { return c->params[c->index.at(name)]; }

struct Mlp2dOff { size_t W, b, g, be; int cin, cout; };
Mlp2dOff up_mlp2d(dsir_ctx* c, Uploader& u, const std::string& pre) {
  const HostParam& w = P(c, pre + ".conv.weight");
  return {u.put(w.data), u.put(P(c, pre + ".conv.bias").data), u.put(P(c, pre + ".norm.weight").data),
          u.put(P(c, pre + ".norm.bias").data), (int)w.shape[1], (int)w.shape[0]};
}
Mlp2dW bind_mlp2d(const float* base, const Mlp2dOff& o) {
  Mlp2dW m;
  m.W = base + o.W; m.b = base + o.b; m.gamma = base + o.g; m.beta = base + o.be;
  m.cin = o.cin; m.cout = o.cout; m.groups = o.cout >= 64 ? 8 : 4;   // RandLANet.py:93
  return m;
}

struct LinOff { size_t W, b; int cin, cout; };
// Conv1d followed (optionally) by eval-mode BatchNorm1d, folded in double precision:
// y = ((W x + b) - mu) / sqrt(var + 1e-5) * g + beta    (RandLANet.py:39-43)
LinOff up_lin(dsir_ctx* c, Uploader& u, const std::string& pre, int pos, bool bn) {
  const HostParam& w = P(c, pre + "." + std::to_string(pos) + ".weight");
  const HostParam& b = P(c, pre + "." + std::to_string(pos) + ".bias");
  const int cout = (int)w.shape[0], cin = (int)w.shape[1];
  std::vector<float> W(w.data), B(b.data);
  if (bn) {
    const std::string q = pre + "." + std::to_string(pos + 1);
    const auto& g = P(c, q + ".weight").data; const auto& be = P(c, q + ".bias").data;
    const auto& mu = P(c, q + ".running_mean").data; const auto& var = P(c, q + ".running_var").data;
    for (int o = 0; o < cout; ++o) {
      const double s = (double)g[o] / std::sqrt((double)var[o] + 1e-5);
      for (int i = 0; i < cin; ++i) W[(size_t)o * cin + i] = (float)((double)w.data[(size_t)o * cin + i] * s);
      B[o] = (float)(((double)b.data[o] - (double)mu[o]) * s + (double)be[o]);
    }
  }
  return {u.put(W), u.put(B), cin, cout};
}
LinW bind_lin(const float* base, const LinOff& o) { LinW l; l.W = base + o.W; l.b = base + o.b; l.cin = o.cin; l.cout = o.cout; return l; }

// Split attentive pooling (d >= 64): G = W1 f is consumed only by the pooling kernel, where lane (fr, fq) of a block needs
// the gathered G values of its column in each of the block's four 16-column tiles.  W1 = fc[:, :d/2] is therefore uploaded
// a second time with its rows permuted so that those four values are adjacent: G' column 64 b + 4 fr + t = the column of
// tile t, lane fr of block b - one 16-byte gather instead of four 4-byte ones.  Which columns form tile t of block b is
// the consumer's mapping: pw_tile.hip (d = 256, the one width Sched::att pools this way: att_keeps_score_cache) takes 64
// consecutive columns.  d = 64 and 128 are still uploaded, in the 32 + 32 pairing of a row-streaming kernel that no longer exists:
// nothing reads them (att_pool.hip pools those levels unsplit), they only keep the blob's layout as it was.
size_t up_fc_g(Uploader& u, const HostParam& fc, int d) {
  if (d < 64) return 0;
  const int h = d / 2;
  std::vector<float> w((size_t)d * h);
  for (int b = 0; b < d / 64; ++b)
    for (int fr = 0; fr < 16; ++fr)
      for (int t = 0; t < 4; ++t) {
        const int pos = 64 * b + 4 * fr + t;
        const int src = d <= 128 ? (t < 2 ? 32 * b + 16 * t + fr : h + 32 * b + 16 * (t - 2) + fr) : 64 * b + 16 * t + fr;
        for (int k = 0; k < h; ++k) w[(size_t)pos * h + k] = fc.data[(size_t)src * d + k];
      }
  return u.put(w);
}

// lse_uv.hip: lfa.mlp1 of a level with d / 2 <= 32 channels, folded for the split by linearity
//   enc_raw[i, k][c] = a[c] dist + U[j][c] + V[i][c]:   per channel {a, ux, uy, uz, vx, vy, vz, b} with u = W[:, 1:4] + W[:, 7:10] (the
// neighbour's coordinates enter through the offset and through their own channels), v = W[:, 4:7] - W[:, 1:4], b = bias.
size_t up_lse_uv(Uploader& u, const HostParam& w, const HostParam& b, int kh) {
  if (kh != 8 && kh != 32) return 0;
  std::vector<float> f((size_t)kh * 8);
  for (int c = 0; c < kh; ++c) {
    const float* r = &w.data[(size_t)c * 10];
    f[c * 8 + 0] = r[0];
    for (int k = 0; k < 3; ++k) { f[c * 8 + 1 + k] = r[1 + k] + r[7 + k]; f[c * 8 + 4 + k] = r[4 + k] - r[1 + k]; }
    f[c * 8 + 7] = b.data[c];
  }
  return u.put(f);
}

struct RandlaOff {
  Mlp2dOff pre, mid, dec[4];
  struct { Mlp2dOff mlp1, lfa1, lfa2, mlp2, skip, a1m, a2m; size_t fc1, fc2, fc1g, fc2g, lse8, pair_w, pair_b; bool pair; } blk[4];
  size_t out_w; int dec_out;
  LinOff fc[3];
};
RandlaOff up_randla(dsir_ctx* c, Uploader& u, const std::string& pre) {
  RandlaOff r;
  r.pre = up_mlp2d(c, u, pre + ".mlp_pre");
  for (int i = 0; i < 4; ++i) {
    const std::string p = pre + ".dilated_res_blocks." + std::to_string(i);
    r.blk[i].mlp1 = up_mlp2d(c, u, p + ".mlp1");
    r.blk[i].lfa1 = up_mlp2d(c, u, p + ".lfa.mlp1");
    r.blk[i].lse8 = up_lse_uv(u, P(c, p + ".lfa.mlp1.conv.weight"), P(c, p + ".lfa.mlp1.conv.bias"), c->cfg.d_out[i] / 2);
    r.blk[i].fc1 = u.put(P(c, p + ".lfa.att_pooling_1.fc.weight").data);
    r.blk[i].fc1g = up_fc_g(u, P(c, p + ".lfa.att_pooling_1.fc.weight"), c->cfg.d_out[i]);
    r.blk[i].a1m = up_mlp2d(c, u, p + ".lfa.att_pooling_1.mlp");
    r.blk[i].lfa2 = up_mlp2d(c, u, p + ".lfa.mlp2");
    r.blk[i].fc2 = u.put(P(c, p + ".lfa.att_pooling_2.fc.weight").data);
    r.blk[i].fc2g = up_fc_g(u, P(c, p + ".lfa.att_pooling_2.fc.weight"), c->cfg.d_out[i]);
    r.blk[i].a2m = up_mlp2d(c, u, p + ".lfa.att_pooling_2.mlp");
    r.blk[i].mlp2 = up_mlp2d(c, u, p + ".mlp2");
    r.blk[i].skip = up_mlp2d(c, u, p + ".mlp_skip");
    // mlp1 and mlp_skip read the same input (RandLANet.py:226 / :229): where mlp1's width is a whole number of 64-column tiles the two
    // weight matrices are uploaded once more, one after the other, for a launch that computes both (GemmArgs::c_split)
    r.blk[i].pair = false; r.blk[i].pair_w = r.blk[i].pair_b = 0;
    {
      const HostParam& w1 = P(c, p + ".mlp1.conv.weight");
      const HostParam& w2 = P(c, p + ".mlp_skip.conv.weight");
      if (w1.shape[0] % 64 == 0 && w1.shape[1] == w2.shape[1]) {
        std::vector<float> w(w1.data), b(P(c, p + ".mlp1.conv.bias").data);
        w.insert(w.end(), w2.data.begin(), w2.data.end());
        const auto& b2 = P(c, p + ".mlp_skip.conv.bias").data;
        b.insert(b.end(), b2.begin(), b2.end());
        r.blk[i].pair_w = u.put(w); r.blk[i].pair_b = u.put(b); r.blk[i].pair = true;
      }
    }
  }
  r.mid = up_mlp2d(c, u, pre + ".mlp_mid");
  for (int j = 0; j < 4; ++j) r.dec[j] = up_mlp2d(c, u, pre + ".decoder_blocks." + std::to_string(j));
  const HostParam& ow = P(c, pre + ".mlp_out.weight");
  r.out_w = u.put(ow.data); r.dec_out = (int)ow.shape[1];
  r.fc[0] = up_lin(c, u, pre + ".fc_label", 0, true);
  r.fc[1] = up_lin(c, u, pre + ".fc_label", 3, true);
  r.fc[2] = up_lin(c, u, pre + ".fc_label", 6, false);
  return r;
}
RandlaW bind_randla(const float* base, const RandlaOff& o, const dsir_cfg& g) {
  RandlaW r;
  r.pre = bind_mlp2d(base, o.pre);
  r.cin = o.pre.cin;
  for (int i = 0; i < 4; ++i) {
    BlockW& b = r.blk[i];
    b.mlp1 = bind_mlp2d(base, o.blk[i].mlp1); b.lfa1 = bind_mlp2d(base, o.blk[i].lfa1);
    b.lfa2 = bind_mlp2d(base, o.blk[i].lfa2); b.mlp2 = bind_mlp2d(base, o.blk[i].mlp2);
    b.skip = bind_mlp2d(base, o.blk[i].skip);
    b.att1.fc = base + o.blk[i].fc1; b.att1.d = g.d_out[i]; b.att1.mlp = bind_mlp2d(base, o.blk[i].a1m);
    b.att2.fc = base + o.blk[i].fc2; b.att2.d = g.d_out[i]; b.att2.mlp = bind_mlp2d(base, o.blk[i].a2m);
    b.att1.fc_g = g.d_out[i] >= 64 ? base + o.blk[i].fc1g : nullptr;
    b.att2.fc_g = g.d_out[i] >= 64 ? base + o.blk[i].fc2g : nullptr;
    b.lse_w8 = (g.d_out[i] == 16 || g.d_out[i] == 64) ? base + o.blk[i].lse8 : nullptr;
    b.d = g.d_out[i]; b.d_in = b.mlp1.cin;
    if (o.blk[i].pair) { b.pair_W = base + o.blk[i].pair_w; b.pair_b = base + o.blk[i].pair_b; }
  }
  r.mid = bind_mlp2d(base, o.mid);
  for (int j = 0; j < 4; ++j) r.dec[j] = bind_mlp2d(base, o.dec[j]);
  r.out_w = base + o.out_w; r.dec_out = o.dec_out;
  for (int k = 0; k < 3; ++k) r.fc[k] = bind_lin(base, o.fc[k]);
  r.ncls = r.fc[2].cout;
  return r;
}

}  // namespace

// fp32 weights -> the two fp16 parts of the split (host side, at weight load; the whole blob: 2.6 M values).  The same loop
// twice: compiled for the baseline x86-64 the fp32 <-> fp16 conversions are library calls (35 ms per load), with F16C they are
// one instruction (2 ms); both round to nearest even, so the parts are the same bits either way.
#define DSIR_SPLIT_LOOP                                 \
  for (size_t i = 0; i < n; ++i) {                      \
    const _Float16 t = (_Float16)w[i];                  \
    const _Float16 l = (_Float16)(w[i] - (float)t);     \
    __builtin_memcpy(hi + i, &t, 2);                    \
    __builtin_memcpy(lo + i, &l, 2);                    \
  }
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__x86_64__)
__attribute__((target("f16c"))) static void split_weights_f16c(const float* w, size_t n, uint16_t* hi, uint16_t* lo) { DSIR_SPLIT_LOOP }
#endif
void split_weights_f16(const float* w, size_t n, uint16_t* hi, uint16_t* lo) {
#if !defined(__HIP_DEVICE_COMPILE__) && defined(__x86_64__)
  if (__builtin_cpu_supports("f16c")) { split_weights_f16c(w, n, hi, lo); return; }
#endif
  DSIR_SPLIT_LOOP
}
#undef DSIR_SPLIT_LOOP

}  // namespace dsir

using namespace dsir;

extern "C" {

int dsir_load_weight(dsir_ctx* c, const char* key, const float* host, const int64_t* shape, int ndim) {
  if (!c || !key) return 1;
  auto it = c->index.find(key);
  if (it == c->index.end()) return fail(c, "unexpected key in state_dict: %s", key);
  HostParam& p = c->params[it->second];
  if (p.ignored) { p.loaded = true; return 0; }
  if (!host) return fail(c, "null data for %s", key);
  if (ndim != (int)p.shape.size()) return fail(c, "size mismatch for %s: expected %d dims, got %d", key, (int)p.shape.size(), ndim);
  for (int d = 0; d < ndim; ++d)
    if (shape[d] != p.shape[d]) return fail(c, "size mismatch for %s: dim %d is %lld, expected %lld", key, d, (long long)shape[d], (long long)p.shape[d]);
  p.data.assign(host, host + p.numel());
  p.loaded = true;
  c->finalized = false;
  return 0;
}

int dsir_finalize_weights(dsir_ctx* c) {
  if (!c) return 1;
  for (auto& p : c->params)
    if (!p.loaded && !p.ignored) return fail(c, "missing key in state_dict: %s", p.name.c_str());
  Uploader u;
  const bool has_agg = c->cfg.pipeline != DSIR_PIPELINE_LABEL, has_inl = c->cfg.pipeline == DSIR_PIPELINE_ALIGN;
  RandlaOff fo = up_randla(c, u, "feat_extractor");
  RandlaOff io{};
  if (has_inl) io = up_randla(c, u, "inlier_model");
  LinOff mf[3] = {}, ma[5] = {}, mp{};
  if (has_agg) {
    mf[0] = up_lin(c, u, "mlp_feat", 0, true); mf[1] = up_lin(c, u, "mlp_feat", 3, true); mf[2] = up_lin(c, u, "mlp_feat", 6, false);
    ma[0] = up_lin(c, u, "mlp_att", 0, true); ma[1] = up_lin(c, u, "mlp_att", 3, true); ma[2] = up_lin(c, u, "mlp_att", 6, true);
    ma[3] = up_lin(c, u, "mlp_att", 9, true); ma[4] = up_lin(c, u, "mlp_att", 12, false);
    mp = up_lin(c, u, "mlp_proj", 0, false);
  }
  HIP_OK(c, hipSetDevice(c->device));
  HIP_OK(c, hipStreamSynchronize(c->stream));
  // a captured registration holds the addresses of the old weight blob: drop it, the next call re-captures
  c->drop_graphs();
  if (c->dweights) { hipFree(c->dweights); c->dweights = nullptr; }
  HIP_OK(c, hipMalloc((void**)&c->dweights, u.blob.size() * sizeof(float)));
  HIP_OK(c, hipMemcpy(c->dweights, u.blob.data(), u.blob.size() * sizeof(float), hipMemcpyHostToDevice));
  const float* b = c->dweights;
  c->net.feat = bind_randla(b, fo, c->cfg);
  if (has_inl) c->net.inl = bind_randla(b, io, c->cfg);
  c->net.feat.ppf = c->net.inl.ppf = (c->flags & DSIR_FLAG_PPF) != 0;
  if (c->dweights16) { hipFree(c->dweights16); c->dweights16 = nullptr; }
  for (int k = 0; k < 5; ++k) c->agg_wh[k] = c->agg_wl[k] = nullptr;
  if (has_agg) {
    for (int k = 0; k < 3; ++k) c->net.mlp_feat[k] = bind_lin(b, mf[k]);
    for (int k = 0; k < 5; ++k) c->net.mlp_att[k] = bind_lin(b, ma[k]);
    c->net.mlp_proj = bind_lin(b, mp);
  }
  {
    // fp16 split (x -> fp16(x), fp16(x - fp16(x))) of the WHOLE blob (BatchNorm already folded), at the same offsets: the kernels
    // with an fp16-split contraction (agg_chain.hip, head_mlp.hip, pw_tile.hip) find the two parts of any matrix W at
    // dweights16 + (W - dweights) and dweights16 + nweights + (W - dweights).  20 MB for the align pipeline.
    u.blob.resize((u.blob.size() + 63) & ~(size_t)63, 0.f);     // the low parts start at dweights16 + total: keep them 16-byte aligned too
    const size_t total = u.blob.size();
    std::vector<uint16_t> h16(2 * total, 0);
    split_weights_f16(u.blob.data(), total, h16.data(), h16.data() + total);
    HIP_OK(c, hipMalloc((void**)&c->dweights16, h16.size() * sizeof(uint16_t)));
    HIP_OK(c, hipMemcpy(c->dweights16, h16.data(), h16.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    c->nweights = total;
    // layers whose matrix the split does not carry run in exact fp32: split_of (schedule.hip) consults this list, the chains
    // that take all their matrices split or none (agg_chain.hip, head_mlp.hip) are decided here
    c->split_off.clear();
    for (const auto& s : u.spans)
      if (!split_in_domain(u.blob.data() + s.first, h16.data() + s.first, h16.data() + total + s.first, s.second - s.first))
        c->split_off.push_back(s);
    auto hi = [&](size_t off) -> const void* { return c->dweights16 + off; };
    auto lo = [&](size_t off) -> const void* { return c->dweights16 + total + off; };
    if (has_agg) {
      const LinOff* lay[5] = {&ma[1], &ma[2], &ma[3], &ma[4], &mp};
      bool ok = true;
      for (int k = 0; k < 5; ++k) ok = ok && c->split_ok(lay[k]->W);
      for (int k = 0; k < 5 && ok; ++k) { c->agg_wh[k] = hi(lay[k]->W); c->agg_wl[k] = lo(lay[k]->W); }
    }
    auto head = [&](const RandlaOff& o, RandlaW& w) {
      bool ok = c->split_ok(o.out_w);
      for (int k = 0; k < 3; ++k) ok = ok && c->split_ok(o.fc[k].W);
      for (int k = 0; k < 4; ++k) w.head_wh[k] = w.head_wl[k] = nullptr;
      if (!ok) return;
      w.head_wh[0] = hi(o.out_w); w.head_wl[0] = lo(o.out_w);
      for (int k = 0; k < 3; ++k) { w.head_wh[k + 1] = hi(o.fc[k].W); w.head_wl[k + 1] = lo(o.fc[k].W); }
    };
    head(fo, c->net.feat);
    if (has_inl) head(io, c->net.inl);
  }
  c->finalized = true;
  return 0;
}

}  // extern "C"
