// Max backward (DGL GSpMM.backward: scatter_add_ through the argmax records): the grouped
// pack / pull form, the argmax-record gather over the transposed CSR it falls back to, the
// DGL-form atomic scatter, and the records' source ids. Work decomposition and numerics:
// spmm_common.hpp.
#include "spmm_common.hpp"
#include "x3_split.hpp"

namespace {

constexpr int kPackWaveMax = 256;  // longest row grouped by one wave (forward chunk)

// ---- max backward, deterministic gather over the transposed CSR ----------------------
// Wave per source row u: for every out-edge (u -> v) at in-row position p (ascending v),
// read v's argmax record; features whose winner is p take dout[v, f] (* w). The record
// loads of U edges are issued together, then their dout loads together (lanes with no
// match read row 0 at the same column instead of branching: a cache hit, no divergence).
template <int W, int NC, bool HAS_W, typename A>
__global__ __launch_bounds__(kBlock) void max_bwd_kernel(
    const float* __restrict__ ew, const int32_t* __restrict__ tcol,
    const int32_t* __restrict__ tslot, const int32_t* __restrict__ tpos,
    const int4* __restrict__ items, int n_items, const A* __restrict__ arg, int64_t lda,
    const float* __restrict__ dout, int64_t ldd, int F, const float* __restrict__ mask,
    int64_t ldm, float* __restrict__ dx, int64_t ldx, float* __restrict__ ws, int64_t ldw) {
  constexpr int U = EdgeU<W, NC>::value;
  const int it = blockIdx.x * kWavesPerBlock + wave_id_uniform();
  if (it >= n_items) return;
  const int4 item = items[it];
  const int row = item.x, t0 = item.y, t1 = item.z, slot = item.w;
  const int lane = lane_id();

  float acc[NC][W];
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int i = 0; i < W; ++i) acc[c][i] = 0.f;

  for (int tw = t0; tw < t1; tw += kWave) {
    const int nw = min(kWave, t1 - tw);
    const int tl = tw + min(lane, nw - 1);
    const int vv = tcol[tl];
    const int pv = tpos[tl];
    float wv = 1.f;
    if constexpr (HAS_W) wv = ew[tslot[tl]];
    for (int j = 0; j < nw; j += U) {
      const int nv = min(U, nw - j);
      int a[U][NC][W];
#pragma unroll
      for (int e = 0; e < U; ++e) {
        const A* ar = arg + (int64_t)bcast(vv, j + min(e, nv - 1)) * lda;
#pragma unroll
        for (int c = 0; c < NC; ++c) load_arg<W, A>(ar, (c * kWave + lane) * W, F, a[e][c]);
      }
      float d[U][NC][W];
#pragma unroll
      for (int e = 0; e < U; ++e) {
        const int je = j + min(e, nv - 1);
        const int p = bcast(pv, je);
        const float* dr = dout + (int64_t)bcast(vv, je) * ldd;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          bool any = false;
#pragma unroll
          for (int i = 0; i < W; ++i) any |= (a[e][c][i] == p);
          load_tile<W>(any ? dr : dout, (c * kWave + lane) * W, F, d[e][c], 0.f);
        }
      }
#pragma unroll
      for (int e = 0; e < U; ++e) {
        if (e < nv) {
          const int p = bcast(pv, j + e);
          float w = 1.f;
          if constexpr (HAS_W) w = bcastf(wv, j + e);
#pragma unroll
          for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int i = 0; i < W; ++i)
              if (a[e][c][i] == p) acc[c][i] += HAS_W ? w * d[e][c][i] : d[e][c][i];
        }
      }
    }
  }

  if (slot < 0) {
    float* xr = dx + (int64_t)row * ldx;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int f = (c * kWave + lane) * W;
      if (mask) {
        float mk[W];
        load_tile<W>(mask + (int64_t)row * ldm, f, F, mk, 0.f);
#pragma unroll
        for (int i = 0; i < W; ++i)
          if (!(mk[i] > 0.f)) acc[c][i] = 0.f;
      }
      store_tile<W>(xr, f, F, acc[c]);
    }
  } else {
    float* wr = ws + (int64_t)slot * ldw;
#pragma unroll
    for (int c = 0; c < NC; ++c) store_tile<W>(wr, (c * kWave + lane) * W, F, acc[c]);
  }
}

// ---- max backward, grouped form (default for u16 records and F <= 1024) ---------------
// Pass 1 (pack), per destination row v: group v's live entries (v, f) by their winning
// in-row position p, giving
//   rec[v F + i]    = {w * dout[v,f], f}, grouped by p (any order inside a group; 8-B
//                     records, or 4-B {bf16 dout, f} for bf16 storage without weights),
//   glist[s]        = start_p | count_p << 16 for the edge at in-CSR slot s = ptr[v] + p:
//                     4 B, the start relative to the row's run v F (a row's descriptors are
//                     contiguous: coalesced stores).
// Rows of in-degree <= kPackWaveMax: one wave per row (wave-private LDS histogram, wave
// scan, LDS-atomic placement); longer rows: one workgroup per row (block histogram, or a
// bitonic sort of (p << 16 | f) keys past kHistMax entries).
// Pass 2 (pull), one wave per source row item: for each out-edge of u, ascending
// destination v (the transposed CSR order), read its descriptor glist[tslot[t]] and add
// its records into an LDS row accumulator (max_bwd_pull_kernel). Traffic per edge: its
// 4-B slot and destination (coalesced), one 4-B descriptor (random; 8 B {v F + start,
// count} before: twice the footprint for the caches to hold) and one short contiguous run
// of records (~F/deg entries).
// Transposed descriptors (round 5; when the caller gives the in-CSR slots' transposed
// indices, g->epos): the descriptor of slot s is stored at its transposed index einv[s],
// and only for edges that win something (about half win nothing: their descriptors stay
// the zero the launch clears the array to). The pull then reads its out-edges' descriptors
// in order, coalesced, and fetches lists only for the edges that have one: one random
// access per live edge instead of two per edge. (Round 3 stored every descriptor at the
// transposed index, empty ones included: pull 35.6 vs 43.5 us, pack 28.3 vs 15.9 us at
// F = 256, no gain. A source-ordered record layout, DESIGN.md §7, measured slower still.)
constexpr int kHistMax = 4096;
constexpr int kGroupMaxF = 1024;  // (starts and counts <= F fit the descriptor's 16-bit halves)

__device__ __forceinline__ uint32_t desc_make(int start, int count) {
  return (uint32_t)start | ((uint32_t)count << 16);
}

// Where the pack puts a descriptor: at the in-CSR slot (TR = false), or at the slot's
// transposed index when the list is not empty (TR = true; the array was cleared first).
template <bool TR>
struct DescOut {
  uint32_t* glist;
  const int32_t* einv;
  // the transposed index of slot s, loaded ahead of the write (TR only)
  __device__ __forceinline__ int pre(int s) const {
    if constexpr (TR) return einv[s];
    else return s;
  }
  __device__ __forceinline__ void put(int pre_s, int start, int count) const {
    if constexpr (TR) {
      if (count > 0) glist[pre_s] = desc_make(start, count);
    } else {
      glist[pre_s] = desc_make(start, count);
    }
  }
};

// one record per list entry, one contiguous run per list (one line for the pull to fetch
// where two arrays cost two). GPack: {value f32, feature u32} (8 B); the value carries the
// edge weight already (w * dout[v,f], the product the pull formed before). GPack4 (bf16
// storage without edge weights): the bf16 upstream gradient itself and the feature,
// {value bf16, feature u16} (4 B); exact, since the value is a bf16 number.
struct GPack {
  using W = uint2;
  W* __restrict__ r;
  __device__ static __forceinline__ W make(int f, float d) { return make_uint2(__float_as_uint(d), (uint32_t)f); }
  __device__ __forceinline__ void put(int64_t pos, int f, float d) const { r[pos] = make(f, d); }
  __device__ __forceinline__ void get(int64_t pos, int& f, float& d) const {
    const W x = r[pos];
    d = __uint_as_float(x.x);
    f = (int)x.y;
  }
};
struct GPack4 {
  using W = uint32_t;
  W* __restrict__ r;
  __device__ static __forceinline__ W make(int f, float d) {
    return (__float_as_uint(d) & 0xFFFF0000u) | (uint32_t)f;
  }
  __device__ __forceinline__ void put(int64_t pos, int f, float d) const { r[pos] = make(f, d); }
  __device__ __forceinline__ void get(int64_t pos, int& f, float& d) const {
    const W x = r[pos];
    d = __uint_as_float(x & 0xFFFF0000u);
    f = (int)(x & 0xFFFFu);
  }
};

// inclusive prefix sum over the 64 lanes: DPP row shifts, then row broadcasts 15 and 31
// (six VALU ops; the __shfl_up form is six dependent ds_bpermute round trips)
__device__ __forceinline__ int wave_incl_add(int x) {
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);  // row_shr:1
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);  // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);  // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);  // row_shr:8
  x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);  // row_bcast:15
  x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);  // row_bcast:31
  return x;
}

__device__ int block_exclusive_scan(int* s, int n, int* wsum) {
  const int per = (n + kBlock - 1) / kBlock;
  const int b = threadIdx.x * per;
  const int lane = lane_id(), wave = threadIdx.x >> 6;
  int local = 0;
  for (int i = 0; i < per; ++i)
    if (b + i < n) local += s[b + i];
  int x = local;
  x = wave_incl_add(x);
  if (lane == kWave - 1) wsum[wave] = x;
  __syncthreads();
  int pre = 0;
  for (int w = 0; w < wave; ++w) pre += wsum[w];
  int run = pre + x - local;
  for (int i = 0; i < per; ++i)
    if (b + i < n) {
      const int t = s[b + i];
      s[b + i] = run;
      run += t;
    }
  const int total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  return total;
}

template <typename A, typename T, typename R, typename D>
__device__ __forceinline__ void pack_short_row(
    int v, int wave, const int32_t* __restrict__ ptr,
    const A* __restrict__ arg, int64_t lda, int F, const T* __restrict__ dout, int64_t ldd,
    const T* __restrict__ fout, int64_t ldf, const float* __restrict__ ew, R gp, D dsc,
    int* __restrict__ lds) {
  constexpr int MAXW = kGroupMaxF / kWave;  // features per lane
  const int lane = lane_id();
  // every independent load first: the row bounds, the argmax record and the upstream
  // gradient (each lane its own features, coalesced), then the list descriptors' slots
  const int rs = ptr[v];
  const int re = ptr[v + 1];
  const A* ar = arg + (int64_t)v * lda;
  const T* dr = dout + (int64_t)v * ldd;
  int a[MAXW];
  float d[MAXW];
#pragma unroll
  for (int i = 0; i < MAXW; ++i) {
    const int f = lane + i * kWave;
    a[i] = f < F ? (int)ar[f] : arg_none<A>();
    d[i] = f < F ? to_f(dr[f]) : 0.f;
  }
  if (fout) {  // a zero maximum: its winner's relu mask is 0, the entry contributes nothing
    const T* fr = fout + (int64_t)v * ldf;
    float m[MAXW];
#pragma unroll
    for (int i = 0; i < MAXW; ++i) m[i] = to_f(fr[min(lane + i * kWave, F - 1)]);
#pragma unroll
    for (int i = 0; i < MAXW; ++i)
      if (m[i] == 0.f) a[i] = arg_none<A>();
  }
  const int deg = re - rs;
  if (deg > kPackWaveMax || deg == 0) return;
  const int B = (deg + kWave - 1) / kWave;  // bins per lane, <= 4
  int ei[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = lane * B + q;
    ei[q] = dsc.pre((q < B && p < deg) ? rs + p : rs);
  }
  int* hist = lds + wave * (kPackWaveMax + 4);
  for (int p = lane; p < deg; p += kWave) hist[p] = 0;
  wave_lds_sync();
#pragma unroll
  for (int i = 0; i < MAXW; ++i)
    if (a[i] != arg_none<A>()) atomicAdd(&hist[a[i]], 1);
  wave_lds_sync();
  // exclusive scan over the deg bins: lane owns bins [lane B, lane B + B)
  int c[4], local = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = lane * B + q;
    c[q] = (q < B && p < deg) ? hist[p] : 0;
    local += c[q];
  }
  int x = local;
  x = wave_incl_add(x);
  int run = x - local;
  const int vF = v * F;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = lane * B + q;
    if (q < B && p < deg) {
      hist[p] = run;
      dsc.put(ei[q], run, c[q]);
      run += c[q];
    }
  }
  wave_lds_sync();
  // placement: every winner straight to its list slot (the order inside a list is free)
#pragma unroll
  for (int i = 0; i < MAXW; ++i)
    if (a[i] != arg_none<A>()) {
      const int pos = vF + atomicAdd(&hist[a[i]], 1);
      gp.put(pos, lane + i * kWave, ew ? ew[rs + a[i]] * d[i] : d[i]);
    }
}

// The same for F <= 256 NV with rows of 4-aligned features: lane l owns the features
// 256 c + 4 l + i (c < NV, i < 4), loaded 4 at a time (argmax records 8 B, upstream
// gradient and forward output 16 B or 8 B), and one LDS atomic per live feature both
// counts its winning position and ranks it inside that position's list (the order inside
// a list is free); the list offsets come from one wave scan over the positions. The lists
// are assembled in LDS and copied out with coalesced stores (scattered 2-B global stores
// are read-modify-writes of partial lines): -6 % for the whole backward on cfg2.
template <int NV>
constexpr int pack_wave_ints() { return kPackWaveMax + 4 + NV * 512; }  // hist | records (8 B)

template <int NV, typename A, typename T, typename R, typename D>
__device__ __forceinline__ void pack_short_row_v(
    int v, int wave, const int32_t* __restrict__ ptr,
    const A* __restrict__ arg, int64_t lda, int F, const T* __restrict__ dout, int64_t ldd,
    const T* __restrict__ fout, int64_t ldf, const float* __restrict__ ew, R gp, D dsc,
    int* __restrict__ lds) {
  const int lane = lane_id();
  const int rs = ptr[v];
  const int deg = ptr[v + 1] - rs;
  if (deg > kPackWaveMax || deg == 0) return;
  int a[NV][4];
  float d[NV][4];
  // straight-line loads at clamped columns (F % 4 == 0 here), masked afterwards: no branch
  // between the record and gradient loads, so both are in flight before the first wait
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    const int f = (c * kWave + lane) * 4;
    const int fc = min(f, F - 4);
    int ac[4];
    float dc[4];
    load_arg<4, A>(arg + (int64_t)v * lda, fc, F, ac);
    load_tile<4, T>(dout + (int64_t)v * ldd, fc, F, dc, 0.f);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[c][i] = f < F ? ac[i] : arg_none<A>();
      d[c][i] = f < F ? dc[i] : 0.f;
    }
  }
  if (fout) {  // a zero maximum: its winner's relu mask is 0, the entry contributes nothing
#pragma unroll
    for (int c = 0; c < NV; ++c) {
      float m[4];
      load_tile<4, T>(fout + (int64_t)v * ldf, (c * kWave + lane) * 4, F, m, 1.f);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (m[i] == 0.f) a[c][i] = arg_none<A>();
    }
  }
  const int B = (deg + kWave - 1) / kWave;  // bins per lane, <= 4
  int ei[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = lane * B + q;
    ei[q] = dsc.pre((q < B && p < deg) ? rs + p : rs);
  }
  int* hist = lds + wave * pack_wave_ints<NV>();
  typename R::W* lr = reinterpret_cast<typename R::W*>(hist + kPackWaveMax + 4);  // 16-B aligned: 260 ints
  for (int p = lane; p < deg; p += kWave) hist[p] = 0;
  wave_lds_sync();
  int rank[NV][4];
#pragma unroll
  for (int c = 0; c < NV; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      rank[c][i] = a[c][i] != arg_none<A>() ? atomicAdd(&hist[a[c][i]], 1) : 0;
  wave_lds_sync();
  int cq[4], local = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = lane * B + q;
    cq[q] = (q < B && p < deg) ? hist[p] : 0;
    local += cq[q];
  }
  int x = local;
  x = wave_incl_add(x);
  int run = x - local;
  const int vF = v * F;
  wave_lds_sync();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = lane * B + q;
    if (q < B && p < deg) {
      hist[p] = run;
      dsc.put(ei[q], run, cq[q]);
      run += cq[q];
    }
  }
  wave_lds_sync();
  if (ew) {  // the edge weight folded into the value: w * d, the product the pull formed
#pragma unroll
    for (int c = 0; c < NV; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) d[c][i] = ew[rs + (a[c][i] != arg_none<A>() ? a[c][i] : 0)] * d[c][i];
  }
#pragma unroll
  for (int c = 0; c < NV; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (a[c][i] != arg_none<A>()) {
        const int pos = hist[a[c][i]] + rank[c][i];
        lr[pos] = R::make((c * kWave + lane) * 4 + i, d[c][i]);
      }
  wave_lds_sync();
  const int total = __builtin_amdgcn_readlane(x, kWave - 1);
  // 16-B stores of 2 (8-B) or 4 (4-B) records per lane (vF and the LDS image are 16-B
  // aligned: F % 4 == 0)
  constexpr int RP = 16 / sizeof(typename R::W);
  for (int i = lane * RP; i < total; i += RP * kWave) {
    if (i + RP <= total) {
      *reinterpret_cast<uint4*>(gp.r + vF + i) = *reinterpret_cast<const uint4*>(lr + i);
    } else {
      for (int k = i; k < total; ++k) gp.r[vF + k] = lr[k];
    }
  }
}

template <typename A, typename T, typename R, typename D>
__device__ __forceinline__ void pack_long_row(
    int v, const int32_t* __restrict__ ptr,
    const A* __restrict__ arg, int64_t lda, int F, const T* __restrict__ dout, int64_t ldd,
    const T* __restrict__ fout, int64_t ldf, const float* __restrict__ ew, R gp, D dsc,
    int* __restrict__ lds) {
  int* hist = lds;
  uint16_t* feats = reinterpret_cast<uint16_t*>(lds + kHistMax + 8);
  int* wsum = lds + kHistMax + 8 + kGroupMaxF / 2;
  const int rs = ptr[v];
  const int deg = ptr[v + 1] - rs;
  if (deg <= kPackWaveMax) return;
  const A* ar = arg + (int64_t)v * lda;
  const int64_t vF = (int64_t)v * F;
  int total;
  if (deg <= kHistMax) {
    // independent loads first (each thread its own features), placement straight to the
    // list slots as in the wave form
    constexpr int FPT = kGroupMaxF / kBlock;
    const T* dr = dout + (int64_t)v * ldd;
    int a[FPT];
    float d[FPT];
#pragma unroll
    for (int i = 0; i < FPT; ++i) {
      const int f = threadIdx.x + i * kBlock;
      a[i] = f < F ? (int)ar[f] : arg_none<A>();
      d[i] = f < F ? to_f(dr[f]) : 0.f;
    }
    if (fout) {  // zero maxima contribute nothing (their winner's relu mask is 0)
      const T* fr = fout + (int64_t)v * ldf;
      float m[FPT];
#pragma unroll
      for (int i = 0; i < FPT; ++i) m[i] = to_f(fr[min((int)threadIdx.x + i * kBlock, F - 1)]);
#pragma unroll
      for (int i = 0; i < FPT; ++i)
        if (m[i] == 0.f) a[i] = arg_none<A>();
    }
    for (int p = threadIdx.x; p < deg; p += kBlock) hist[p] = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < FPT; ++i)
      if (a[i] != arg_none<A>()) atomicAdd(&hist[a[i]], 1);
    __syncthreads();
    total = block_exclusive_scan(hist, deg, wsum);
    for (int p0 = threadIdx.x; p0 < deg; p0 += 4 * kBlock) {
      int e[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int p = p0 + j * kBlock;
        e[j] = dsc.pre(p < deg ? rs + p : rs);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int p = p0 + j * kBlock;
        if (p < deg) {
          const int st = hist[p];
          const int en = p + 1 < deg ? hist[p + 1] : total;
          dsc.put(e[j], st, en - st);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < FPT; ++i)
      if (a[i] != arg_none<A>()) {
        const int64_t pos = vF + atomicAdd(&hist[a[i]], 1);
        gp.put(pos, threadIdx.x + i * kBlock, ew ? ew[rs + a[i]] * d[i] : d[i]);
      }
    return;
  } else {
    // hub row: bitonic sort of (p << 16 | f) keys; "none" sorts last
    uint32_t* keys = reinterpret_cast<uint32_t*>(hist);
    int np = 1;
    while (np < F) np <<= 1;
    for (int i = threadIdx.x; i < np; i += kBlock) {
      uint32_t key = 0xFFFFFFFFu;
      if (i < F) {
        const int a = (int)ar[i];
        const bool live = !fout || to_f(fout[(int64_t)v * ldf + i]) != 0.f;
        if (a != arg_none<A>() && live) key = ((uint32_t)a << 16) | (uint32_t)i;
      }
      keys[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= np; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = threadIdx.x; i < np; i += kBlock) {
          const int ixj = i ^ j;
          if (ixj > i) {
            const uint32_t a = keys[i], b = keys[ixj];
            if ((a > b) == ((i & k) == 0)) {
              keys[i] = b;
              keys[ixj] = a;
            }
          }
        }
        __syncthreads();
      }
    auto lower = [&](uint32_t key) {
      int lo = 0, hi = np;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
      }
      return lo;
    };
    for (int p = threadIdx.x; p < deg; p += kBlock) {
      const int es = dsc.pre(rs + p);
      const int st = lower((uint32_t)p << 16);
      const int en = lower((uint32_t)(p + 1) << 16);
      dsc.put(es, st, en - st);
    }
    if (threadIdx.x == 0) wsum[0] = lower(0xFFFFFFFFu);
    __syncthreads();
    total = wsum[0];
    for (int i = threadIdx.x; i < total; i += kBlock) feats[i] = (uint16_t)(keys[i] & 0xFFFFu);
    __syncthreads();
  }
  const T* dr = dout + (int64_t)v * ldd;
  for (int i = threadIdx.x; i < total; i += kBlock) {
    const int f = feats[i];
    const float dv = to_f(dr[f]);
    gp.put(vF + i, f, ew ? ew[rs + (int)(reinterpret_cast<const uint32_t*>(hist)[i] >> 16)] * dv : dv);
  }
}

// One launch for both: blocks [0, n_long) take the rows past kPackWaveMax (`rows` lists
// them, as {row, ...} int4 = the split-row merges of a schedule whose chunk is <=
// kPackWaveMax; NULL = every row, short ones exit at once) so the long rows start first;
// the remaining blocks take 4 rows each, one wave per row.
constexpr int kPackLds = kHistMax + 8 + kGroupMaxF / 2 + 4;
static_assert(kPackLds >= kWavesPerBlock * (kPackWaveMax + 4), "pack LDS");

// ACT (pg_spmm_max_bwd_rows): a destination row with row_active[v] == 0 counts as dout = 0
// and is left out whole: no loads of its dout / arg rows, no records, no descriptors (the
// wave, or the long row's workgroup, returns at once). Its lists would carry only +-0
// values, which change no bit of a sum that starts at +0.
template <typename A, typename T, int NV, typename R, bool TR, bool ACT = false>
__global__ __launch_bounds__(kBlock) void group_pack_kernel(
    const int4* __restrict__ rows, int n_long, int n_rows, const int32_t* __restrict__ ptr,
    const A* __restrict__ arg, int64_t lda, int F,
    const T* __restrict__ dout, int64_t ldd, const T* __restrict__ fout, int64_t ldf,
    const float* __restrict__ ew, R gp, uint32_t* __restrict__ glist, const int32_t* __restrict__ einv,
    uint32_t* __restrict__ tickets, int n_tickets, const int8_t* __restrict__ row_active) {
  // the pull's split-row ticket counters start every call at zero (this launch precedes it)
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n_tickets; i += gridDim.x * kBlock) tickets[i] = 0u;
  const DescOut<TR> dsc{glist, einv};
  constexpr int kLds = NV > 0 && kWavesPerBlock * pack_wave_ints<NV>() > kPackLds
                           ? kWavesPerBlock * pack_wave_ints<NV>() : kPackLds;
  __shared__ __attribute__((aligned(16))) int lds[kLds];
  const int b = blockIdx.x;
  if (b < n_long) {
    const int v = rows ? rows[b].x : b;
    if constexpr (ACT)
      if (!row_active[v]) return;  // (block-uniform)
    pack_long_row<A, T, R>(v, ptr, arg, lda, F, dout, ldd, fout, ldf, ew, gp, dsc, lds);
  } else {
    const int wave = wave_id_uniform();
    const int v = (b - n_long) * kWavesPerBlock + wave;
    if (v < n_rows)
    {
      if constexpr (ACT)
        if (!row_active[v]) return;  // (wave-uniform; the short-row forms have no block barrier)
      if constexpr (NV > 0)
        pack_short_row_v<NV, A, T, R>(v, wave, ptr, arg, lda, F, dout, ldd, fout, ldf, ew, gp, dsc, lds);
      else
        pack_short_row<A, T, R>(v, wave, ptr, arg, lda, F, dout, ldd, fout, ldf, ew, gp, dsc, lds);
    }
  }
}

#ifndef PG_PULL_MERGE
#define PG_PULL_MERGE 1  // split rows combined inside the pull (0: the sum_merge_kernel launch)
#endif

#ifndef PG_PULL_U
#define PG_PULL_U 8  // list segments in flight per wave (4-8 best on S0, 16 +6 %, 32 +25 %)
#endif

// Pass 2 (pull): one wave per source-row item {u, t0, t1, slot}, its out-edges in windows
// of 64 (ascending destination); lane j holds window edge j's descriptor (loaded through its
// in-CSR slot tslot[t]: the descriptors one window ahead, the slots two). The records of
// each list are added into an LDS row accumulator. A list never repeats a feature, so the
// lanes of one segment add into distinct words, and every feature's terms are summed in
// ascending v, the order of the sequential scatter_add_ (bit-exact on rows that are not
// split across items). Dense segments across several lists, added in order by LDS
// compare-and-swap (the float LDS atomic, ds_add_f32, runs at 1/16 of the integer atomics'
// rate on gfx950: scripts/probes/lds_rmw_probe.hip), measured slower on the engine's data:
// a source that wins a feature at many destinations puts it many times into one segment,
// and the swaps serialise.
// In-launch combine of split rows (MERGE; replaces sum_merge_kernel's launch): the pieces of a
// row longer than the schedule's chunk store their partial rows write-through (sc1), drain
// them, and draw a ticket from the row's counter (one per first slot, zeroed by the pack);
// the piece that draws the last ticket reads every slot of the row with sc1 loads (no stale
// L1 or other-XCD L2 line can serve them, so no acquire fence) and sums them in slot order
// from +0, exactly sum_merge_kernel's order: the same bits whichever piece arrives last.
struct PullMerge {
  const int32_t* ptr;  // the transposed CSR's row pointers (piece index = (t0 - ptr[row]) / chunk)
  int chunk;           // the schedule's chunk (pg_schedule_build)
  uint32_t* tickets;   // [n_slots]
  uint32_t ws_bytes;   // the slot region (< 2 GiB, checked on the host)
};


// ACT (pg_spmm_max_bwd_rows, descriptors at the in-CSR slots): `tslot` is the caller's
// eslot_active, -1 at every out-edge whose destination row is inactive. Such an edge has no
// list (the pack wrote it no descriptor): its descriptor load still runs, at slot 0, outside
// every branch (so the waits stay counted), and its count is taken as 0 where it is used.
template <typename T, typename R, bool TR, bool MERGE, bool ACT = false>
__global__ __launch_bounds__(kBlock) void max_bwd_pull_kernel(
    const int32_t* __restrict__ tslot, const int4* __restrict__ items, int n_items,
    const int32_t* __restrict__ tdst, const uint32_t* __restrict__ glist, R gp, int F,
    const T* __restrict__ mask, int64_t ldm, T* __restrict__ dx, int64_t ldx, float* __restrict__ ws,
    int64_t ldw, PullMerge pm) {
  constexpr int U = PG_PULL_U;
  __shared__ __attribute__((aligned(16))) float accs[kWavesPerBlock][kGroupMaxF];
  const int wave = wave_id_uniform();
  const int it = blockIdx.x * kWavesPerBlock + wave;
  if (it >= n_items) return;
  float* acc = accs[wave];
  const int4 item = items[it];
  const int row = item.x, t0 = item.y, t1 = item.z, slot = item.w;
  const int lane = lane_id();
  // (MERGE: the 16-B slot stores cover ldw = round_up(F, 4) columns)
  for (int f = lane; f < (MERGE ? (int)ldw : F); f += kWave) acc[f] = 0.f;
  // descriptors (and the destinations' record bases v F) one window ahead, their in-CSR
  // slots two windows ahead (an item with no out-edges reads nothing)
  auto tl_of = [&](int tw) { return tw + min(lane, t1 - tw - 1); };
  static_assert(!(ACT && TR), "transposed descriptors need no active form: the pack skips the rows");
  uint32_t dsc_next = 0;
  int vf_next = 0, ts_next = 0;
  bool dead_next = false;  // ACT: the descriptor in dsc_next belongs to an inactive row's edge
  // TR: the descriptors sit at the transposed indices themselves (coalesced, no slot loads)
  if (t1 > t0) {
    if constexpr (ACT) {
      const int s = tslot[tl_of(t0)];
      dead_next = s < 0;
      dsc_next = glist[max(s, 0)];
    } else {
      dsc_next = glist[TR ? tl_of(t0) : tslot[tl_of(t0)]];
    }
    vf_next = tdst[tl_of(t0)] * F;
    if (!TR && t0 + kWave < t1) ts_next = tslot[tl_of(t0 + kWave)];
  }
  for (int tw = t0; tw < t1; tw += kWave) {
    const int nw = min(kWave, t1 - tw);
    // this window's edge (lane): its list's first record and its length
    const int2 dsc = make_int2(vf_next + (int)(dsc_next & 0xFFFFu),
                               ACT && dead_next ? 0 : (int)(dsc_next >> 16));
    if (tw + kWave < t1) {
      if constexpr (ACT) {
        dead_next = ts_next < 0;
        dsc_next = glist[max(ts_next, 0)];
      } else {
        dsc_next = glist[TR ? tl_of(tw + kWave) : ts_next];
      }
      vf_next = tdst[tl_of(tw + kWave)] * F;
      if (!TR && tw + 2 * kWave < t1) ts_next = tslot[tl_of(tw + 2 * kWave)];
    }
    // segments: 64-entry pieces of single lists, U segments' loads in flight. Segment t
    // belongs to the edge i with excl_i <= t < excl_i + nseg_i, i.e.
    // i = popcount(ballot(excl <= t)) - 1.
    {
      const int nseg = lane < nw ? (dsc.y + kWave - 1) / kWave : 0;
      const int incl = wave_incl_add(nseg);
      const int excl = incl - nseg;
      const int nseg_all = bcast(incl, kWave - 1);
      for (int s0 = 0; s0 < nseg_all; s0 += U) {
        const int nv = min(U, nseg_all - s0);
        int fe[U], ne[U];
        float de[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int t = s0 + min(u, nv - 1);
          const int i = __popcll(__ballot(excl <= t)) - 1;
          const int seg = t - bcast(excl, i);
          const int base = bcast(dsc.x, i) + seg * kWave;
          const int n = min(kWave, bcast(dsc.y, i) - seg * kWave);
          ne[u] = n;
          // straight-line loads (lanes past n load a valid entry of the same segment), so
          // the waits are counted instead of a vmcnt(0) behind each branch
          gp.get(base + min(lane, n - 1), fe[u], de[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (u < nv && lane < ne[u]) acc[fe[u]] += de[u];
      }
    }
  }
  wave_lds_sync();
  if (slot < 0) {
    T* xr = dx + (int64_t)row * ldx;
    const T* mr = mask ? mask + (int64_t)row * ldm : nullptr;
    for (int f = lane; f < F; f += kWave) {
      float a = acc[f];
      if (mr && !(to_f(mr[f]) > 0.f)) a = 0.f;
      xr[f] = from_f<T>(a);
    }
  } else if constexpr (MERGE) {
    const __amdgpu_buffer_rsrc_t rs = pg_x3::rsrc(ws, pm.ws_bytes);
    const uint32_t sbase = (uint32_t)slot * (uint32_t)ldw * 4u;
    for (int f = lane * 4; f < F; f += kWave * 4)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(pg_u32x4, *reinterpret_cast<const float4*>(acc + f)), rs, sbase + (uint32_t)f * 4u,
                                             0, 16);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every payload store drained before the ticket
    const int rb = pm.ptr[row], re = pm.ptr[row + 1];
    const int s0 = slot - (t0 - rb) / pm.chunk;
    const int ns = (re - rb + pm.chunk - 1) / pm.chunk;
    uint32_t ticket = 0;
    if (lane == 0)
      ticket = __hip_atomic_fetch_add((pg_gu32*)(pm.tickets + s0), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ticket = __builtin_amdgcn_readfirstlane(ticket);
    if ((int)ticket != ns - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // keeps the loads below the ticket
    T* xr = dx + (int64_t)row * ldx;
    const T* mr = mask ? mask + (int64_t)row * ldm : nullptr;
    for (int f = lane * 4; f < F; f += kWave * 4) {
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      for (int s = s0; s < s0 + ns; s += 8) {
        float4 v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          v[e] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
              rs, (uint32_t)min(s + e, s0 + ns - 1) * (uint32_t)ldw * 4u + (uint32_t)f * 4u, 0, 16));
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (s + e < s0 + ns) {
            a[0] += v[e].x; a[1] += v[e].y; a[2] += v[e].z; a[3] += v[e].w;
          }
      }
      if (mr) {
        float mk[4];
        load_tile<4, T>(mr, f, F, mk, 0.f);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (!(mk[i] > 0.f)) a[i] = 0.f;
      }
      store_tile<4, T>(xr, f, F, a);
    }
  } else {
    float* wr = ws + (int64_t)slot * ldw;
    for (int f = lane; f < F; f += kWave) wr[f] = acc[f];
  }
}

// ---- DGL-form scatter backward (float atomics) ----------------------------------------
template <typename A, bool HAS_W>
__global__ __launch_bounds__(kBlock) void max_bwd_scatter_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
    const int32_t* __restrict__ eslot, const float* __restrict__ ew, int64_t n_rows,
    const A* __restrict__ arg, int64_t lda, const float* __restrict__ dout, int64_t ldd, int F,
    float* __restrict__ dx, int64_t ldx) {
  const int64_t row = (int64_t)blockIdx.x * kWavesPerBlock + wave_id_uniform();
  if (row >= n_rows) return;
  const int rs = ptr[row];
  for (int f = lane_id(); f < F; f += kWave) {
    const int a = (int)arg[row * lda + f];
    if (a == arg_none<A>()) continue;
    const int k = rs + a;
    const int u = col[k];
    float d = dout[row * ldd + f];
    if (HAS_W) d = ew[eslot ? eslot[k] : k] * d;
    atomicAdd(dx + (int64_t)u * ldx + f, d);
  }
}

template <typename A>
__global__ __launch_bounds__(kBlock) void argpos_to_src_kernel(
    const int32_t* __restrict__ ptr, const int32_t* __restrict__ col, int64_t n_rows,
    const A* __restrict__ arg, int64_t lda, int F, int64_t* __restrict__ argx, int64_t ldx) {
  const int64_t n = n_rows * (int64_t)F;
  for (int64_t i = blockIdx.x * (int64_t)kBlock + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kBlock) {
    const int64_t v = i / F;
    const int f = (int)(i - v * F);
    const int a = (int)arg[v * lda + f];
    argx[v * ldx + f] = a == arg_none<A>() ? -1 : (int64_t)col[ptr[v] + a];
  }
}

template <typename A>
int launch_max_bwd(const pg_csr_t* g, const pg_csr_t* gt, const A* arg, int64_t lda,
                   const float* dout, int64_t ldd, int64_t F, const float* mask, int64_t ldm,
                   float* dx, int64_t ldx, float* ws, int64_t ldw, hipStream_t st) {
  TilePlan tp = plan_tiles(F, {lda, ldd, ldx, mask ? ldm : 4}, {dout, dx, mask, ws});
  if (tp.vec && ((uintptr_t)arg & (4 * sizeof(A) - 1)) != 0) tp.vec = false;
  if (!tp.vec) tp.tile = kFTileScalar;
  const bool has_w = g->ew != nullptr;
  const int blocks = grid_for(gt->n_items);
  for (int64_t f0 = 0; f0 < F; f0 += tp.tile) {
    const int Ft = (int)std::min<int64_t>(tp.tile, F - f0);
    auto go = [&](auto nc_c, auto w_c, auto hw_c) -> int {
      constexpr int NC = decltype(nc_c)::value;
      constexpr int W = decltype(w_c)::value;
      constexpr bool HW = decltype(hw_c)::value;
      hipLaunchKernelGGL((max_bwd_kernel<W, NC, HW, A>), dim3(blocks), dim3(kBlock), 0, st,
                         g->ew, gt->col, gt->eslot, gt->epos, (const int4*)gt->items,
                         (int)gt->n_items, arg + f0, lda, dout + f0, ldd, Ft,
                         mask ? mask + f0 : nullptr, ldm, dx + f0, ldx, ws ? ws + f0 : nullptr,
                         ldw);
      return PG_OK;
    };
    const int rc = dispatch_tile(tp, Ft, has_w, go);
    if (rc != PG_OK) return pg::set_error(rc, "pg_spmm_max_bwd: unsupported feature tile");
    if (gt->n_merges > 0) {
      hipLaunchKernelGGL(sum_merge_kernel<float>, dim3((unsigned)gt->n_merges), dim3(kBlock), 0, st,
                         (const int4*)gt->merges, (int)gt->n_merges, Ft, ws + f0, ldw, gt->ptr, 0,
                         mask ? mask + f0 : nullptr, ldm, dx + f0, ldx);
    }
  }
  return hip_status("pg_spmm_max_bwd");
}

// [split-row partials][grouped path: list records N x F x 8 B | glist nnz x 4 B | tickets n_slots x 4 B]
inline size_t bwd_partials_bytes(const pg_csr_t* gt, int64_t F) {
  return gt->n_slots > 0 ? round_up(gt->n_slots * ws_ld(F) * 4, 256) : 0;
}

template <typename T>
int max_bwd_entry(const pg_csr_t* g, const pg_csr_t* gt, const void* argpos, int64_t lda,
                  int arg_kind, const T* dout, int64_t ldd, int64_t F, const T* mask_src,
                  int64_t ldm, const T* fwd_out, int64_t ldf, T* dx, int64_t ldx, void* ws,
                  size_t ws_bytes, pg_stream_t stream, const int8_t* row_active = nullptr,
                  const int32_t* eslot_active = nullptr) {
  PG_TRY(pg::check_csr(g, "pg_spmm_max_bwd", false));
  PG_TRY(pg::check_csr(gt, "pg_spmm_max_bwd", true));
  // PG_ARG_DEAD_NONE: the records already leave out the zero maxima (fwd_out's filter)
  const bool dead_none = (arg_kind & PG_ARG_DEAD_NONE) != 0;
  arg_kind &= ~PG_ARG_DEAD_NONE;
  if (!pg::valid_arg_kind(arg_kind))
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_bwd: bad arg_kind %d", arg_kind);
  if (gt->n_cols != g->n_rows || gt->nnz != g->nnz)
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_bwd: gt is not the transpose of g");
  if (gt->nnz > 0 && (!gt->epos || !gt->eslot))
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_bwd: gt needs eslot and epos");
  if (F < 0 || ldd < F || ldx < F || lda < F || (mask_src && ldm < F) || (fwd_out && ldf < F))
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_bwd: bad F/leading dims");
  if ((fwd_out || dead_none) && !mask_src)
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_bwd: fwd_out / PG_ARG_DEAD_NONE needs mask_src");
  if (dead_none) fwd_out = nullptr;
  if (F == 0 || gt->n_rows == 0) return pg::ok();
  if (!argpos || !dout || !dx) return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_bwd: NULL buffer");
  // active rows (pg_spmm_max_bwd_rows): both arrays or neither
  const bool act = row_active != nullptr;
  if (act != (eslot_active != nullptr))
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_bwd_rows: row_active and eslot_active go together");
  const size_t need = pg_spmm_max_bwd_workspace(gt, F);
  PG_TRY(check_ws(ws_bytes, need, "pg_spmm_max_bwd"));
  // every region below starts a multiple of 256 B past ws: the records (uint2, 16-B copies),
  // the descriptors' uint4 clear and the partial rows' 16-B slot accesses inherit ws's alignment
  if (need > 0 && !aligned16(ws))
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_bwd: ws must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t pbytes = bwd_partials_bytes(gt, F);
  float* w = pbytes ? (float*)ws : nullptr;
  const int64_t N = g->n_rows;
  if (arg_kind == PG_ARG_U16 && F <= kGroupMaxF && N * F < INT32_MAX) {
    char* p = (char*)ws + pbytes;
    // the records carry the upstream gradient as f32 (8 B), or for bf16 storage without edge
    // weights as its bf16 value (4 B); the sums are f32 either way (one rounding of dx at the
    // end, as the oracle's f32 sums)
    void* recs = p;
    p += round_up(N * F * 8, 256);
    uint32_t* glist = (uint32_t*)p;
    p += round_up(g->nnz * 4, 256);
    uint32_t* tickets = (uint32_t*)p;
    // split rows combined inside the pull (sum_merge_kernel's launch otherwise): vector rows,
    // the schedule's chunk known, a slot region a 32-bit buffer offset covers
    constexpr uintptr_t kTm = 4 * sizeof(T) - 1;
    const bool merge_in = PG_PULL_MERGE && gt->n_merges > 0 && gt->chunk > 0 && F % 4 == 0 && ldx % 4 == 0 &&
                          ((uintptr_t)dx & kTm) == 0 && ((uintptr_t)w & 15) == 0 && pbytes < ((size_t)1 << 31) &&
                          (!mask_src || dead_none || (ldm % 4 == 0 && ((uintptr_t)mask_src & kTm) == 0));
    const int n_tickets = merge_in ? (int)gt->n_slots : 0;
    const auto* arg16 = (const uint16_t*)argpos;
    // rows past kPackWaveMax: the schedule's split rows when its chunk guarantees they are
    // a superset, else every row
    const bool listed = g->merges != nullptr && g->chunk > 0 && g->chunk <= kPackWaveMax;
    const int n_long = (int)(listed ? g->n_merges : N);
    const int n_short_blocks = (int)((N + kWavesPerBlock - 1) / kWavesPerBlock);
    // 4 features per lane (vector loads) when every row is 4-aligned
    constexpr uintptr_t kTa = 4 * sizeof(T) - 1;
    const bool vec = F % 4 == 0 && lda % 4 == 0 && ldd % 4 == 0 && (!fwd_out || ldf % 4 == 0) &&
                     ((uintptr_t)argpos & 7) == 0 && ((uintptr_t)dout & kTa) == 0 && ((uintptr_t)fwd_out & kTa) == 0;
    const dim3 pgrid((unsigned)(n_long + n_short_blocks));
    const int4* prow = listed ? (const int4*)g->merges : nullptr;
    // transposed descriptors when the in-CSR slots' transposed indices are given (g->epos)
    const bool tr = g->epos != nullptr && ((uintptr_t)glist & 15) == 0;
    // cleared by a kernel of this library, not hipMemsetAsync: a memset issued while the
    // stream is being captured into a HIP graph did not clear the array on replays (the
    // engine's step graph trained on stale descriptors)
    if (tr && g->nnz > 0) {
      const int64_t n4 = (g->nnz + 3) / 4;  // glist is 256-B aligned and padded: whole uint4s
      hipLaunchKernelGGL(clear_u4_kernel, dim3((unsigned)std::min<int64_t>(2048, (n4 + kBlock - 1) / kBlock)),
                         dim3(kBlock), 0, st, reinterpret_cast<uint4*>(glist), n4);
    }
    auto run = [&](auto gp, auto tr_c) {
    using R = decltype(gp);
    constexpr bool TR = decltype(tr_c)::value;
    auto pack = [&](auto nv_c) {
      constexpr int NV = decltype(nv_c)::value;
      if (act)
        hipLaunchKernelGGL((group_pack_kernel<uint16_t, T, NV, R, TR, true>), pgrid, dim3(kBlock), 0, st, prow,
                           n_long, (int)N, g->ptr, arg16, lda, (int)F, dout, ldd, fwd_out, ldf, g->ew, gp, glist,
                           g->epos, tickets, n_tickets, row_active);
      else
        hipLaunchKernelGGL((group_pack_kernel<uint16_t, T, NV, R, TR, false>), pgrid, dim3(kBlock), 0, st, prow,
                           n_long, (int)N, g->ptr, arg16, lda, (int)F, dout, ldd, fwd_out, ldf, g->ew, gp, glist,
                           g->epos, tickets, n_tickets, (const int8_t*)nullptr);
      return PG_OK;
    };
    if (vec) dispatch_nc<kGroupMaxF / 256>((int)((F + 255) / 256), pack);
    else pack(std::integral_constant<int, 0>{});
    const int blocks = grid_for(gt->n_items);
    // dead-none records imply the relu' mask (the contract: mask_src >= 0): every entry left
    // in the lists has a maximum X[u,f] w != 0, so X[u,f] > 0; an element with no entries
    // sums to +0, which the mask would leave +0. With fwd_out alone the mask is applied.
    if (dead_none) mask_src = nullptr;
    const PullMerge pm{gt->ptr, gt->chunk, tickets, (uint32_t)pbytes};
    // active rows with the descriptors at the in-CSR slots: the pull reads eslot_active (the
    // inactive rows' descriptors were not written). Transposed descriptors: the array was
    // cleared and the pack wrote the active rows' live edges only, so the pull is the plain one.
    auto pull = [&](auto merge_c, auto act_c) {
      constexpr bool MG = decltype(merge_c)::value, AC = decltype(act_c)::value;
      hipLaunchKernelGGL((max_bwd_pull_kernel<T, R, TR, MG, AC>), dim3(blocks), dim3(kBlock), 0, st,
                         AC ? eslot_active : gt->eslot, (const int4*)gt->items, (int)gt->n_items, gt->col, glist,
                         gp, (int)F, mask_src, ldm, dx, ldx, w, ws_ld(F), pm);
    };
    if constexpr (!TR) {
      if (act) {
        if (merge_in) pull(std::true_type{}, std::true_type{});
        else pull(std::false_type{}, std::true_type{});
      } else {
        if (merge_in) pull(std::true_type{}, std::false_type{});
        else pull(std::false_type{}, std::false_type{});
      }
    } else {
      if (merge_in) pull(std::true_type{}, std::false_type{});
      else pull(std::false_type{}, std::false_type{});
    }
    if (gt->n_merges > 0 && !merge_in)
      hipLaunchKernelGGL(sum_merge_kernel<T>, dim3((unsigned)gt->n_merges), dim3(kBlock), 0, st,
                         (const int4*)gt->merges, (int)gt->n_merges, (int)F, w, ws_ld(F), gt->ptr, 0,
                         mask_src, ldm, dx, ldx);
    };
    auto run_tr = [&](auto gp) {
      if (tr) run(gp, std::true_type{});
      else run(gp, std::false_type{});
    };
    if constexpr (sizeof(T) == 2) {  // (f32 storage has no 4-B record form)
      if (!g->ew) {
        run_tr(GPack4{(uint32_t*)recs});
        return hip_status("pg_spmm_max_bwd");
      }
    }
    run_tr(GPack{(uint2*)recs});
    return hip_status("pg_spmm_max_bwd");
  }
  if (act)
    return pg::set_error(PG_ERR_UNSUPPORTED, "pg_spmm_max_bwd_rows: needs PG_ARG_U16 records and F <= %d (grouped path)",
                         kGroupMaxF);
  if constexpr (sizeof(T) == 4) {
    if (arg_kind == PG_ARG_U16)
      return launch_max_bwd<uint16_t>(g, gt, (const uint16_t*)argpos, lda, dout, ldd, F, mask_src,
                                      ldm, dx, ldx, w, ws_ld(F), st);
    return launch_max_bwd<int32_t>(g, gt, (const int32_t*)argpos, lda, dout, ldd, F, mask_src, ldm,
                                   dx, ldx, w, ws_ld(F), st);
  } else {
    return pg::set_error(PG_ERR_UNSUPPORTED,
                         "pg_spmm_max_bwd_bf16: needs PG_ARG_U16 records and F <= %d (grouped path)",
                         kGroupMaxF);
  }
}

}  // namespace

extern "C" {

size_t pg_spmm_max_bwd_workspace(const pg_csr_t* gt, int64_t F) {
  if (!gt || F <= 0) return 0;
  size_t b = bwd_partials_bytes(gt, F);
  if (F <= kGroupMaxF) {
    const int64_t N = gt->n_cols;
    b += round_up(N * F * 8, 256) + round_up(gt->nnz * 4, 256);
    if (gt->n_slots > 0) b += round_up(gt->n_slots * 4, 256);  // the pull's split-row tickets
  }
  return b;
}

int pg_spmm_max_bwd(const pg_csr_t* g, const pg_csr_t* gt, const void* argpos, int64_t lda,
                    int arg_kind, const float* dout, int64_t ldd, int64_t F,
                    const float* mask_src, int64_t ldm, const float* fwd_out, int64_t ldf,
                    float* dx, int64_t ldx, void* ws, size_t ws_bytes, pg_stream_t stream) {
  return max_bwd_entry<float>(g, gt, argpos, lda, arg_kind, dout, ldd, F, mask_src, ldm, fwd_out, ldf,
                              dx, ldx, ws, ws_bytes, stream);
}

int pg_spmm_max_bwd_bf16(const pg_csr_t* g, const pg_csr_t* gt, const void* argpos, int64_t lda,
                         int arg_kind, const void* dout, int64_t ldd, int64_t F,
                         const void* mask_src, int64_t ldm, const void* fwd_out, int64_t ldf,
                         void* dx, int64_t ldx, void* ws, size_t ws_bytes, pg_stream_t stream) {
  return max_bwd_entry<uint16_t>(g, gt, argpos, lda, arg_kind, (const uint16_t*)dout, ldd, F,
                                 (const uint16_t*)mask_src, ldm, (const uint16_t*)fwd_out, ldf,
                                 (uint16_t*)dx, ldx, ws, ws_bytes, stream);
}

int pg_spmm_max_bwd_rows(const pg_csr_t* g, const pg_csr_t* gt, const void* argpos, int64_t lda,
                         int arg_kind, const float* dout, int64_t ldd, int64_t F,
                         const float* mask_src, int64_t ldm, const float* fwd_out, int64_t ldf,
                         float* dx, int64_t ldx, const int8_t* row_active, const int32_t* eslot_active,
                         void* ws, size_t ws_bytes, pg_stream_t stream) {
  return max_bwd_entry<float>(g, gt, argpos, lda, arg_kind, dout, ldd, F, mask_src, ldm, fwd_out, ldf,
                              dx, ldx, ws, ws_bytes, stream, row_active, eslot_active);
}

int pg_spmm_max_bwd_rows_bf16(const pg_csr_t* g, const pg_csr_t* gt, const void* argpos, int64_t lda,
                              int arg_kind, const void* dout, int64_t ldd, int64_t F,
                              const void* mask_src, int64_t ldm, const void* fwd_out, int64_t ldf,
                              void* dx, int64_t ldx, const int8_t* row_active, const int32_t* eslot_active,
                              void* ws, size_t ws_bytes, pg_stream_t stream) {
  return max_bwd_entry<uint16_t>(g, gt, argpos, lda, arg_kind, (const uint16_t*)dout, ldd, F,
                                 (const uint16_t*)mask_src, ldm, (const uint16_t*)fwd_out, ldf,
                                 (uint16_t*)dx, ldx, ws, ws_bytes, stream, row_active, eslot_active);
}

int pg_spmm_max_bwd_scatter(const pg_csr_t* g, const void* argpos, int64_t lda, int arg_kind,
                            const float* dout, int64_t ldd, int64_t F, float* dx, int64_t ldx,
                            int64_t n_src, pg_stream_t stream) {
  PG_TRY(pg::check_csr(g, "pg_spmm_max_bwd_scatter", false));
  if (!pg::valid_arg_kind(arg_kind))
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_bwd_scatter: bad arg_kind %d", arg_kind);
  if (F < 0 || ldd < F || ldx < F || lda < F || n_src < g->n_cols)
    return pg::set_error(PG_ERR_INVALID, "pg_spmm_max_bwd_scatter: bad F/leading dims");
  if (F == 0) return pg::ok();
  hipStream_t st = (hipStream_t)stream;
  const int64_t n_fill = n_src * F;
  const int fill_blocks = (int)std::min<int64_t>(4096, (n_fill + kBlock - 1) / kBlock);
  if (fill_blocks > 0)
    hipLaunchKernelGGL(fill2d_kernel, dim3(fill_blocks), dim3(kBlock), 0, st, dx, ldx, n_src,
                       (int)F, 0.f);
  const int blocks = grid_for(g->n_rows);
  if (blocks > 0) {
    const bool hw = g->ew != nullptr;
    if (arg_kind == PG_ARG_U16) {
      if (hw)
        hipLaunchKernelGGL((max_bwd_scatter_kernel<uint16_t, true>), dim3(blocks), dim3(kBlock), 0, st,
                           g->ptr, g->col, g->eslot, g->ew, g->n_rows, (const uint16_t*)argpos, lda,
                           dout, ldd, (int)F, dx, ldx);
      else
        hipLaunchKernelGGL((max_bwd_scatter_kernel<uint16_t, false>), dim3(blocks), dim3(kBlock), 0, st,
                           g->ptr, g->col, g->eslot, g->ew, g->n_rows, (const uint16_t*)argpos, lda,
                           dout, ldd, (int)F, dx, ldx);
    } else {
      if (hw)
        hipLaunchKernelGGL((max_bwd_scatter_kernel<int32_t, true>), dim3(blocks), dim3(kBlock), 0, st,
                           g->ptr, g->col, g->eslot, g->ew, g->n_rows, (const int32_t*)argpos, lda,
                           dout, ldd, (int)F, dx, ldx);
      else
        hipLaunchKernelGGL((max_bwd_scatter_kernel<int32_t, false>), dim3(blocks), dim3(kBlock), 0, st,
                           g->ptr, g->col, g->eslot, g->ew, g->n_rows, (const int32_t*)argpos, lda,
                           dout, ldd, (int)F, dx, ldx);
    }
  }
  return hip_status("pg_spmm_max_bwd_scatter");
}

int pg_argpos_to_src(const pg_csr_t* g, const void* argpos, int64_t lda, int arg_kind,
                     int64_t F, int64_t* argx, int64_t ldx, pg_stream_t stream) {
  PG_TRY(pg::check_csr(g, "pg_argpos_to_src", false));
  if (!pg::valid_arg_kind(arg_kind))
    return pg::set_error(PG_ERR_INVALID, "pg_argpos_to_src: bad arg_kind %d", arg_kind);
  if (F < 0 || lda < F || ldx < F)
    return pg::set_error(PG_ERR_INVALID, "pg_argpos_to_src: bad F/leading dims");
  const int64_t n = g->n_rows * F;
  if (n == 0) return pg::ok();
  const int blocks = (int)std::min<int64_t>(4096, (n + kBlock - 1) / kBlock);
  hipStream_t st = (hipStream_t)stream;
  if (arg_kind == PG_ARG_U16)
    hipLaunchKernelGGL((argpos_to_src_kernel<uint16_t>), dim3(blocks), dim3(kBlock), 0, st, g->ptr,
                       g->col, g->n_rows, (const uint16_t*)argpos, lda, (int)F, argx, ldx);
  else
    hipLaunchKernelGGL((argpos_to_src_kernel<int32_t>), dim3(blocks), dim3(kBlock), 0, st, g->ptr,
                       g->col, g->n_rows, (const int32_t*)argpos, lda, (int)F, argx, ldx);
  return hip_status("pg_argpos_to_src");
}

}  // extern "C"
