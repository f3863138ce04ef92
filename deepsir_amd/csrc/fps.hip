// Farthest-point sampling of a batch of clouds: dsir_farthest_point_sample (include/dsir.h), Engine.farthest_point_sample.  What the
// reference does on the host in dataloader/data_base.py:328 (farthest_point_sampler) and with a loop of torch ops in
// network/tools.py:30 (farthest_point_sample), and open3d's farthest_point_down_sample.  open3d cannot be imported here, so parity is
// unpinned and THE RULE IS OWNED HERE; deepsir_amd/fps.py restates it in numpy (farthest_point_sample_host).
//
// ---- THE RULE.  Inputs: points [clouds][cap][stride >= 3] fp32; counts [clouds] i32 or none: cloud c has n = clamp(counts[c], 0, cap)
// rows (none: cap), rows at and past n are never read; k >= 1; start >= 0.
//   Arithmetic: fp32, every operation rounded on its own (no contraction).  d = p_i - p_c per coordinate,
//     d2(i, c) = (dx dx + dy dy) + dz dz, as icp.hip and overlap.hip form it.
//   Eligibility: a row with a non-finite coordinate is never a candidate and never selected; a selected row is never selected again.
//   Selection: s_0 = start if start < n and that row is finite, else the lowest finite row.  For t >= 1:
//     dist_i = min(dist_i, d2(i, s_(t-1))) over the remaining candidates, from dist_i = +inf;  s_t = the candidate of largest dist,
//     ties to the lower index.  No candidate left: the cloud ends with count_out = t.
//   Outputs: index [clouds][k] i32 in selection order, -1 beyond count_out; counts_out [clouds] i32; min_d2 [clouds][k] fp32, the dist
//     of s_t when it was chosen: +inf for s_0, 0 beyond count_out, non-increasing in t by construction.
//   Nothing depends on the launch, the batch composition or timing; no atomics.  (The reference functions differ in two ways: they
//   draw s_0 at random, and they do not exclude selected rows - whose dist is 0, so they return only once every dist is 0.)
//
// ---- Kernel shape (fps.h holds the key, the row-to-lane map, the tiers and the scratch layout; tools/fps_check.cpp checks them).
// One workgroup per cloud, grid = clouds; the k steps run inside the kernel, no host round trip, no workgroup waits on another.
// Row i lives in lane i % T, register slot i / T, for the whole call; a slot whose rows all lie past n is skipped (a uniform branch).
// Candidate key = (bits(dist) << 32) | (0xffffffff - i), one u64 per candidate, 0 for a row that is none (dist = -1 marks it in
// the registers: non-finite, past n, or selected).  Step 0 is the same reduction on dist = +inf with `start` lifted one above.
// Per step: each lane updates its rows and keeps its largest dist (strictly larger only: the lower slot keeps a tie) with that row's
// coordinates, one key per lane; the wave's max by an xor butterfly of
// __shfl_xor on the u64 (6 steps); the lane that holds it writes key and coordinates to the wave's LDS slot, so the next step needs no
// dependent global load; slots are double-buffered by step parity: ONE __syncthreads() per step; every wave then reduces the W
// slots redundantly (lane l reads slot l % W, log2 W butterfly steps) and reads the winner's coordinates from the slot of the wave
// that owns it; lane 0 of the workgroup writes index[t] and min_d2[t], the owning lane retires the row.  The max of u64 keys is
// exact and order-free, so the bytes depend on neither T nor the tier.
//   register tiers: cap <= 1024 -> T = 256, 4 slots (one wave per SIMD: the step is latency, not work); cap <= 8192 -> T = 1024, 8
//     slots.  Coordinates and dist in registers; the loop touches global memory only to write index and min_d2.
//   streaming tier: 8192 < cap <= 65536 -> T = 1024, 64 dist registers per lane, coordinates re-read each step from the float4-packed
//     copy FpsLayout::xyz4 (a lane reads back only rows it packed itself, so the copy needs no barrier), 16 B rows (the compiler loads the 12 B it uses, global_load_dwordx3), 4 in flight
//     per lane, no per-row test (the copy holds zero rows up to a whole group of slots).  cap > 65536 is refused by the entry.
// Build (-Rpass-analysis=kernel-resource-usage, gfx950):
//   fps_kernel<256, 4, false>    54 VGPRs, 46 SGPRs,  256 B LDS, no scratch, 8 waves per SIMD allowed (4 waves run)
//   fps_kernel<1024, 8, false>   78 VGPRs, 60 SGPRs, 1024 B LDS, no scratch, 6 waves per SIMD allowed (the workgroup is 4 per SIMD)
//   fps_kernel<1024, 64, true>  105 VGPRs, 70 SGPRs, 1024 B LDS, no scratch, 4 waves per SIMD (a 1024-thread workgroup caps a lane at 128
//     registers, not 512: hence four loads in flight, not more, and the slot addresses formed per step - hoisted out of the step
//     loop the 64 of them spilled)
// Open costs: the step is a chain of cross-lane exchanges (6 + log2 W butterfly steps through ds_bpermute, two per u64) and one
// barrier; DPP row operations for the first four steps would shorten it.  One workgroup per cloud leaves the other 255 CUs idle on a
// single cloud: several workgroups per cloud need cross-workgroup synchronisation per step and are out of scope.
#include "device_utils.h"
#include "fps.h"
#include "kernels.h"

namespace dsir {

namespace {

struct alignas(16) FpsSlot { unsigned long long key; float x, y, z, pad; };

template <int N> __device__ __forceinline__ unsigned long long fps_butterfly_max(unsigned long long m) {
#pragma unroll
  for (int o = N / 2; o >= 1; o >>= 1) {
    const unsigned long long p = __shfl_xor(m, o);
    m = p > m ? p : m;
  }
  return m;
}

// The workgroup's part of a step: the lane's largest key and that row's coordinates in; the step's winning key out (0: no candidate
// left; every wave returns the same value) with its coordinates in (cx, cy, cz).  s: the W slots of this step's parity.
template <int T> __device__ __forceinline__ unsigned long long fps_settle(FpsSlot* s, unsigned long long best, float bx, float by, float bz,
                                                                          float& cx, float& cy, float& cz) {
  constexpr int W = T / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long wmax = fps_butterfly_max<64>(best);
  if (best == wmax && (wmax != 0 || lane == 0)) {           // keys are distinct: one lane per wave
    s[wave].key = wmax; s[wave].x = bx; s[wave].y = by; s[wave].z = bz;
  }
  __syncthreads();
  const unsigned long long top = fps_butterfly_max<W>(s[lane & (W - 1)].key);
  if (top != 0) {
    const int w = (int)(fps_key_index(top) % (uint32_t)T) >> 6;       // the wave that owns the winner
    cx = s[w].x; cy = s[w].y; cz = s[w].z;
  }
  return top;
}

// the winner of step t: lane 0 writes it out, the lane that owns the row retires it
template <int T, int R> __device__ __forceinline__ void fps_commit(unsigned long long top, int t, float (&dist)[R], int32_t* out_i, float* out_d) {
  const uint32_t win = fps_key_index(top);
  if (threadIdx.x == 0) {
    out_i[t] = (int32_t)win;
    out_d[t] = __uint_as_float(t == 0 ? kFpsInfBits : fps_key_dist_bits(top));
  }
  const int rw = threadIdx.x == win % (uint32_t)T ? (int)(win / (uint32_t)T) : -1;
#pragma unroll
  for (int r = 0; r < R; ++r) dist[r] = r == rw ? -1.f : dist[r];     // selects on registers: no indexed store
}

template <int T, int R, bool STREAM>
__global__ __launch_bounds__(T) void fps_kernel(const float* __restrict__ pts, int64_t pts_cs, int stride, const int32_t* __restrict__ counts,
                                                int cap, int k, int start, float4* __restrict__ xyz4, int32_t* __restrict__ index,
                                                int32_t* __restrict__ counts_out, float* __restrict__ min_d2) {
  constexpr int W = T / 64;                 // waves = LDS slots per parity
  constexpr int G = STREAM ? kFpsStreamGroup : 1;   // register slots handled together
  static_assert(R % G == 0 && (W & (W - 1)) == 0 && W <= 64, "slot groups and the cross-wave butterfly");
  __shared__ FpsSlot slot[2][W];
  const int cloud = blockIdx.x, tid = threadIdx.x;
  const int n = pair_rows(counts, cloud, cap);
  const int live = fps_live_slots(n, T);    // uniform: slots at and past it hold no row
  const float* P = pts + cloud * pts_cs;
  float4* Q = xyz4 + (int64_t)cloud * fps_stream_rows(cap);        // streaming tier only
  float dist[R];
  float x[STREAM ? 1 : R], y[STREAM ? 1 : R], z[STREAM ? 1 : R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    dist[r] = -1.f;
    float px = 0.f, py = 0.f, pz = 0.f;
    const int i = fps_row(tid, r, T);
    if (r < live && i < n) {
      const float* p = P + (int64_t)i * stride;
      px = p[0]; py = p[1]; pz = p[2];
      if (isfinite(px) && isfinite(py) && isfinite(pz)) dist[r] = __uint_as_float(kFpsInfBits);
    }
    if (STREAM && r < fps_stream_slots(live)) Q[i] = make_float4(px, py, pz, 0.f);        // zeros past n: the loop loads without a test
    if (!STREAM) { x[r] = px; y[r] = py; z[r] = pz; }
  }
  int32_t* out_i = index + (int64_t)cloud * k;
  float* out_d = min_d2 + (int64_t)cloud * k;
  const char* Qc = reinterpret_cast<const char*>(Q);        // slot r of this lane: byte offset tid * 16 + r * (T * 16)
  float cx = 0.f, cy = 0.f, cz = 0.f;
  int t = 0;
  {   // step 0: every finite row has dist = +inf, so the lane's best is its lowest finite slot - or `start`, one above +inf
    const int rs = start % T == tid ? start / T : R;        // the slot of `start` if this lane holds it
    int br = -1;
    float bx = 0.f, by = 0.f, bz = 0.f;
#pragma unroll
    for (int r = R - 1; r >= 0; --r)        // descending: the lowest finite slot stays, unless `start` was met above it
      if (dist[r] >= 0.f && br != rs) {
        br = r;
        if (!STREAM) { bx = x[STREAM ? 0 : r]; by = y[STREAM ? 0 : r]; bz = z[STREAM ? 0 : r]; }
      }
    unsigned long long best = 0;
    if (br >= 0) {
      best = fps_key(br == rs ? kFpsStartBits : kFpsInfBits, (uint32_t)fps_row(tid, br, T));
      if (STREAM) {
        const float4 q = *reinterpret_cast<const float4*>(Qc + ((uint32_t)tid * 16u + (uint32_t)br * (T * 16u)));
        bx = q.x; by = q.y; bz = q.z;
      }
    }
    const unsigned long long top = fps_settle<T>(slot[0], best, bx, by, bz, cx, cy, cz);
    if (top != 0) { fps_commit<T, R>(top, 0, dist, out_i, out_d); t = 1; }
  }
  for (; t >= 1 && t < k; ++t) {
    float bd = -1.f, bx = 0.f, by = 0.f, bz = 0.f;
    int br = 0;
    uint32_t qoff = (uint32_t)tid * 16u;
    if (STREAM) asm volatile("" : "+v"(qoff));              // the 64 slot addresses are formed per step: hoisted out of the loop they spill
#pragma unroll
    for (int rb = 0; rb < R; rb += G) {
      if (rb < live) {
        float px[G], py[G], pz[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          if (STREAM) {
            const float4 q = *reinterpret_cast<const float4*>(Qc + (qoff + (uint32_t)(rb + g) * (T * 16u)));
            px[g] = q.x; py[g] = q.y; pz[g] = q.z;
          } else {
            px[g] = x[STREAM ? 0 : rb + g]; py[g] = y[STREAM ? 0 : rb + g]; pz[g] = z[STREAM ? 0 : rb + g];
          }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const int r = rb + g;
          const float dx = px[g] - cx, dy = py[g] - cy, dz = pz[g] - cz;
          const float d2 = (dx * dx + dy * dy) + dz * dz;
          float d = dist[r];
          d = d2 < d ? d2 : d;              // a NaN d2 (a non-finite row) leaves d = -1; a retired row stays at -1 as d2 >= 0
          dist[r] = d;
          if (d > bd) { bd = d; br = r; bx = px[g]; by = py[g]; bz = pz[g]; }     // strict: the lower slot, i.e. the lower index, keeps a tie
        }
      }
    }
    const unsigned long long best = bd < 0.f ? 0ull : fps_key(__float_as_uint(bd), (uint32_t)fps_row(tid, br, T));
    const unsigned long long top = fps_settle<T>(slot[t & 1], best, bx, by, bz, cx, cy, cz);
    if (top == 0) break;                    // no candidate left: a uniform exit
    fps_commit<T, R>(top, t, dist, out_i, out_d);
  }
  for (int j = t + tid; j < k; j += T) { out_i[j] = -1; out_d[j] = 0.f; }
  if (tid == 0) counts_out[cloud] = t;
}

}  // namespace

size_t fps_scratch_bytes(int clouds, int cap) { return FpsLayout(clouds, cap).bytes; }

bool launch_fps(const FpsArgs& a, hipStream_t st) {
  const FpsPlan p = fps_plan(a.cap);
  if (p.threads == 0 || a.clouds < 1 || a.clouds > 65535 || a.k < 1 || a.k > a.cap || a.start < 0 || a.pts_ld < 3) return false;
  if (!a.pts || !a.index || !a.counts_out || !a.min_d2 || (p.stream && !a.scratch)) return false;
  float4* xyz4 = p.stream ? at<float4>(a.scratch, FpsLayout(a.clouds, a.cap).xyz4) : nullptr;
  const dim3 grid((unsigned)a.clouds);
#define DSIR_FPS_LAUNCH(T, R, S)                                                                                                  \
  hipLaunchKernelGGL((fps_kernel<T, R, S>), grid, dim3(T), 0, st, a.pts, a.pts_cs, a.pts_ld, a.counts, a.cap, a.k, a.start, xyz4, \
                     a.index, a.counts_out, a.min_d2)
  if (p.stream) DSIR_FPS_LAUNCH(1024, 64, true);
  else if (p.threads == 256) DSIR_FPS_LAUNCH(256, 4, false);
  else DSIR_FPS_LAUNCH(1024, 8, false);
#undef DSIR_FPS_LAUNCH
  return true;
}

}  // namespace dsir
