// Nucleus features and centroids from an instance mask ("F4", the first front-end step: dataflow/construct_feature_graph.py:50-123 +
// common/nuc_feature.py).  Three parts:
//   1. label pass over all H*W pixels: per label value the pixel count, bbox and exact int64 row / column sums, aggregated within a
//      wave before one atomic per distinct label of the wave;
//   2. compaction (one workgroup): labels with count < min_size are dropped (skimage 0.15 remove_small_objects on a label image),
//      output rows are assigned in ascending label order by a ballot scan, crops larger than the LDS path are listed for part 3b;
//   3. one workgroup per surviving nucleus computes its 16 features over the crop [r0, r1 + 2) x [c0, c1 + 2) (the reference's crop
//      quirk) -- (a) with every per-crop array in LDS, or (b) for the listed large crops, the same code on a slot of caller-provided
//      global workspace.
// The surviving-foreground test inside a crop is count[label] >= min_size (no second image is written).  Every floating sum runs in
// a fixed order: the output is bitwise reproducible.  The arithmetic, item by item: kernels.py KernelSpec.nucleus_features.
#include <stdint.h>

#include "common.hpp"
#include "image_common.hpp"

#define NUC_LDS_PIXELS 2048           // crops of at most this many pixels take the LDS path (3a)
#define NUC_LDS_SLOTS 8192            // GLCM pair hash (3a), reused afterwards for the contour vertices: = 4 * NUC_LDS_PIXELS
#define NUC_THREADS 256
#define NUC_BIG_SLOTS 32              // workgroups of the global-workspace path (3b)

namespace {

struct LabelTables {                   // carved out of the label-pass workspace; index = label value
  int* cnt;
  int* rmin;
  int* rmax;
  int* cmin;
  int* cmax;
  long long* sr;
  long long* sc;
  int* big_rows;                       // rows of the crops that take path 3b, ascending
  int max_label;
};

static inline LabelTables tables_layout(Carver&& c, int max_label) {      // the one definition of the label-pass workspace
  const int64_t m = (int64_t)max_label + 1;
  LabelTables t;
  t.cnt = c.take<int>(m);
  t.rmin = c.take<int>(m);
  t.rmax = c.take<int>(m);
  t.cmin = c.take<int>(m);
  t.cmax = c.take<int>(m);
  t.sr = c.take<long long>(m);
  t.sc = c.take<long long>(m);
  t.big_rows = c.take<int>(m);
  t.max_label = max_label;
  return t;
}

// crop of label L: rows [r0, r0 + ch), columns [c0, c0 + cw)
__device__ inline int64_t crop_pixels(const LabelTables& t, int L, int H, int W) {
  const int ch = min(t.rmax[L] + 2, H) - t.rmin[L], cw = min(t.cmax[L] + 2, W) - t.cmin[L];
  return (int64_t)ch * cw;
}

__global__ void k_nuc_init(LabelTables t, int* meta) {
  const int64_t m = (int64_t)t.max_label + 1;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
    t.cnt[i] = 0;
    t.rmin[i] = INT32_MAX;
    t.rmax[i] = -1;
    t.cmin[i] = INT32_MAX;
    t.cmax[i] = -1;
    t.sr[i] = 0;
    t.sc[i] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x < 4) meta[threadIdx.x] = 0;
}

template <typename T>
__device__ inline T wave_min(T v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, (T)__shfl_xor(v, o));
  return v;
}
template <typename T>
__device__ inline T wave_max(T v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, (T)__shfl_xor(v, o));
  return v;
}
template <typename T>
__device__ inline T wave_sum(T v) {
  for (int o = 32; o > 0; o >>= 1) v += (T)__shfl_xor(v, o);
  return v;
}

// Part 1.  Consecutive pixels go to consecutive lanes, so a wave sees few distinct labels: per distinct label the lanes holding it
// reduce their contributions across the wave and one lane issues the atomics (cdna_hip_programming.md, Guideline 12).  Labels
// outside [0, max_label] are counted in meta[3] and otherwise ignored.
__global__ void k_nuc_label_pass(const int* __restrict__ labels, int H, int W, LabelTables t, int* meta) {
  const int64_t npix = (int64_t)H * W;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < npix; base += stride) {   // uniform trip count per wave
    const int64_t i = base + threadIdx.x;
    const bool inside = i < npix;
    const int L = inside ? labels[i] : 0;
    const bool bad = inside && (L < 0 || L > t.max_label);
    const uint64_t badm = __ballot(bad);
    if (badm != 0 && lane == 0) atomicAdd(&meta[3], (int)__popcll(badm));
    const bool mine = inside && L > 0 && L <= t.max_label;
    const int r = inside ? (int)(i / W) : 0, c = inside ? (int)(i - (int64_t)r * W) : 0;
    uint64_t todo = __ballot(mine);
    while (todo != 0) {
      const int leader = (int)__builtin_ctzll(todo);
      const int Lw = __shfl(L, leader);
      const bool in = mine && L == Lw;
      const uint64_t grp = __ballot(in);
      const int rmn = wave_min(in ? r : INT32_MAX), rmx = wave_max(in ? r : -1);
      const int cmn = wave_min(in ? c : INT32_MAX), cmx = wave_max(in ? c : -1);
      const long long srs = wave_sum(in ? (long long)r : 0ll), scs = wave_sum(in ? (long long)c : 0ll);
      if (lane == leader) {
        atomicAdd(&t.cnt[Lw], (int)__popcll(grp));
        atomicMin(&t.rmin[Lw], rmn);
        atomicMax(&t.rmax[Lw], rmx);
        atomicMin(&t.cmin[Lw], cmn);
        atomicMax(&t.cmax[Lw], cmx);
        atomicAdd((unsigned long long*)&t.sr[Lw], (unsigned long long)srs);
        atomicAdd((unsigned long long*)&t.sc[Lw], (unsigned long long)scs);
      }
      todo &= ~grp;
    }
  }
}

// Part 2, one workgroup of 1024 threads: ascending label order by a ballot scan, chunk after chunk.
// meta = {rows, large crops, pixels of the largest large crop, refused pixels}.
__global__ void __launch_bounds__(1024) k_nuc_compact(LabelTables t, int H, int W, int min_size, int* __restrict__ kept, int* meta) {
  __shared__ int wtot[2][16];
  __shared__ int run[3];                 // rows so far, large crops so far, largest large crop
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) run[0] = run[1] = run[2] = 0;
  __syncthreads();
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  for (int64_t base = 1; base <= t.max_label; base += 1024) {
    const int64_t L = base + tid;
    const int cnt = L <= t.max_label ? t.cnt[L] : 0;
    const bool keep = cnt > 0 && cnt >= min_size;
    const int64_t px = keep ? crop_pixels(t, (int)L, H, W) : 0;
    const bool big = keep && px > NUC_LDS_PIXELS;
    const uint64_t bk = __ballot(keep), bb = __ballot(big);
    if (lane == 0) {
      wtot[0][w] = (int)__popcll(bk);
      wtot[1][w] = (int)__popcll(bb);
    }
    __syncthreads();
    int ok = 0, ob = 0;
    for (int v = 0; v < w; ++v) {
      ok += wtot[0][v];
      ob += wtot[1][v];
    }
    const int row = run[0] + ok + (int)__popcll(bk & lt);
    if (keep) kept[row] = (int)L;
    if (big) {
      t.big_rows[run[1] + ob + (int)__popcll(bb & lt)] = row;
      atomicMax(&run[2], (int)px);
    }
    __syncthreads();
    if (tid == 0) {
      int sk = 0, sb = 0;
      for (int v = 0; v < 16; ++v) {
        sk += wtot[0][v];
        sb += wtot[1][v];
      }
      run[0] += sk;
      run[1] += sb;
    }
    __syncthreads();
  }
  if (tid == 0) {
    meta[0] = run[0];
    meta[1] = run[1];
    meta[2] = run[2];
  }
}

// ---- part 3: one nucleus per workgroup
struct Red {                             // LDS scratch of the fixed-order block reductions and the two histograms
  long long l[NUC_THREADS];
  double d[NUC_THREADS];
  int hist[256];                         // foreground gray levels of the crop
  int histd[256];                        // |i - j| of the GLCM pairs
};

__device__ inline long long block_sum(long long v, Red& s) {
  const int tid = threadIdx.x;
  s.l[tid] = v;
  __syncthreads();
  for (int o = NUC_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) s.l[tid] += s.l[tid + o];
    __syncthreads();
  }
  const long long r = s.l[0];
  __syncthreads();
  return r;
}
__device__ inline double block_sum(double v, Red& s) {
  const int tid = threadIdx.x;
  s.d[tid] = v;
  __syncthreads();
  for (int o = NUC_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) s.d[tid] += s.d[tid + o];
    __syncthreads();
  }
  const double r = s.d[0];
  __syncthreads();
  return r;
}
__device__ inline long long block_max(long long v, Red& s) {
  const int tid = threadIdx.x;
  s.l[tid] = v;
  __syncthreads();
  for (int o = NUC_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) s.l[tid] = max(s.l[tid], s.l[tid + o]);
    __syncthreads();
  }
  const long long r = s.l[0];
  __syncthreads();
  return r;
}

// skimage.filters.rank.entropy(gray, disk(3)) at one pixel: the histogram of the (up to 29) in-image values under the disk,
// -sum p log2 p in double (distinct values in first-occurrence order).
__device__ inline double local_entropy(const uint8_t* __restrict__ gray, int H, int W, int R, int C) {
  int v[29];
  int k = 0;
#pragma unroll
  for (int dy = -3; dy <= 3; ++dy) {
#pragma unroll
    for (int dx = -3; dx <= 3; ++dx) {
      if (dx * dx + dy * dy > 9) continue;
      const int y = R + dy, x = C + dx;
      v[k++] = (y >= 0 && y < H && x >= 0 && x < W) ? (int)gray[(int64_t)y * W + x] : -1;
    }
  }
  int pop = 0;
#pragma unroll
  for (int j = 0; j < 29; ++j) pop += v[j] >= 0;
  double e = 0.0;
#pragma unroll
  for (int j = 0; j < 29; ++j) {
    int cnt = 0;
    bool first = v[j] >= 0;
#pragma unroll
    for (int q = 0; q < 29; ++q) {
      cnt += v[q] == v[j];
      if (q < j && v[q] == v[j]) first = false;
    }
    if (first) {
      const double p = (double)cnt / (double)pop;
      e -= p * log(p) / 0.6931471805599453;
    }
  }
  return e;
}

// cyclic Jacobi eigen-decomposition of a symmetric k x k matrix (k <= 5); a[] is destroyed, the eigenvalues end on its diagonal
__device__ inline void jacobi_eig(double* a, double* V, int k) {
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) V[i * k + j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0, tot = 0.0;
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < k; ++j) {
        tot += a[i * k + j] * a[i * k + j];
        if (i != j) off += a[i * k + j] * a[i * k + j];
      }
    if (!(off > 1e-32 * tot)) break;
    for (int p = 0; p < k - 1; ++p)
      for (int q = p + 1; q < k; ++q) {
        const double apq = a[p * k + q];
        if (apq == 0.0) continue;
        const double th = (a[q * k + q] - a[p * k + p]) / (2.0 * apq);
        const double tt = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
        for (int r = 0; r < k; ++r) {                   // columns p, q
          const double arp = a[r * k + p], arq = a[r * k + q];
          a[r * k + p] = c * arp - s * arq;
          a[r * k + q] = s * arp + c * arq;
        }
        for (int r = 0; r < k; ++r) {                   // rows p, q
          const double apr = a[p * k + r], aqr = a[q * k + r];
          a[p * k + r] = c * apr - s * aqr;
          a[q * k + r] = s * apr + c * aqr;
        }
        for (int r = 0; r < k; ++r) {
          const double vrp = V[r * k + p], vrq = V[r * k + q];
          V[r * k + p] = c * vrp - s * vrq;
          V[r * k + q] = s * vrp + c * vrq;
        }
      }
  }
}

// minimum-norm solution of the symmetric system M x = b: eigen-directions with |lambda| <= rel * max |lambda| are dropped
__device__ inline void pinv_solve(double* M, const double* b, double* x, int k, double rel) {
  double V[25];
  jacobi_eig(M, V, k);
  double lmax = 0.0;
  for (int i = 0; i < k; ++i) lmax = fmax(lmax, fabs(M[i * k + i]));
  for (int i = 0; i < k; ++i) x[i] = 0.0;
  for (int e = 0; e < k; ++e) {
    const double l = M[e * k + e];
    if (!(fabs(l) > rel * lmax)) continue;
    double proj = 0.0;
    for (int i = 0; i < k; ++i) proj += V[i * k + e] * b[i];
    proj /= l;
    for (int i = 0; i < k; ++i) x[i] += proj * V[i * k + e];
  }
}

struct Scratch {                         // per-crop arrays: LDS (3a) or a slot of global workspace (3b)
  int* comp;                             // [P] smallest raster index of the pixel's 8-connected component (foreground)
  uint8_t* fg;                           // [P] surviving foreground
  uint8_t* outer;                        // [P] background 4-connected to the outside of the crop
  uint32_t* glcm;                        // 3a: NUC_LDS_SLOTS-slot hash (key << 16 | count); 3b: dense [65536] counts
  int* verts;                            // contour vertices as crop pixel indices
  int64_t vcap;
};

template <bool LDS>
__device__ void nucleus(const int* __restrict__ labels, const uint8_t* __restrict__ gray, int H, int W, int min_size, const LabelTables& t,
                        int L, int row, const Scratch& S, Red& sh, float* __restrict__ feat, float* __restrict__ cen, int* __restrict__ info) {
  const int tid = threadIdx.x;
  const int r0 = t.rmin[L], c0 = t.cmin[L];
  const int ch = min(t.rmax[L] + 2, H) - r0, cw = min(t.cmax[L] + 2, W) - c0;
  const int64_t P = (int64_t)ch * cw;
  for (int i = tid; i < 256; i += NUC_THREADS) sh.hist[i] = sh.histd[i] = 0;
  const int nslots = LDS ? NUC_LDS_SLOTS : 65536;
  for (int i = tid; i < nslots; i += NUC_THREADS) S.glcm[i] = 0u;
  __syncthreads();

  // (a) surviving foreground, intensity histogram, background sums, local entropy over the foreground
  long long nbg = 0, sbg = 0;
  double ent = 0.0;
  for (int64_t p = tid; p < P; p += NUC_THREADS) {
    const int y = (int)(p / cw), x = (int)(p - (int64_t)y * cw);
    const int64_t gi = (int64_t)(r0 + y) * W + (c0 + x);
    const int lab = labels[gi];
    const bool f = lab > 0 && lab <= t.max_label && t.cnt[lab] >= min_size;
    const int g = gray[gi];
    S.fg[p] = f;
    S.comp[p] = f ? (int)p : INT32_MAX;
    S.outer[p] = (!f && (y == 0 || x == 0 || y == ch - 1 || x == cw - 1)) ? 1 : 0;
    if (f) {
      atomicAdd(&sh.hist[g], 1);
      ent += local_entropy(gray, H, W, r0 + y, c0 + x);
    } else {
      ++nbg;
      sbg += g;
    }
  }
  __syncthreads();

  // (b) GLCM of gray * mask, offset (0, +1), pairs with both levels > 0 (row and column 0 dropped)
  long long npair = 0, sdis = 0;
  for (int64_t p = tid; p < P; p += NUC_THREADS) {
    const int y = (int)(p / cw), x = (int)(p - (int64_t)y * cw);
    if (x + 1 >= cw || !S.fg[p] || !S.fg[p + 1]) continue;
    const int64_t gi = (int64_t)(r0 + y) * W + (c0 + x);
    const int a = gray[gi], b = gray[gi + 1];
    if (a == 0 || b == 0) continue;
    ++npair;
    const int d = a > b ? a - b : b - a;
    sdis += d;
    atomicAdd(&sh.histd[d], 1);
    const uint32_t key = ((uint32_t)a << 8) | (uint32_t)b;    // >= 257: a taken slot is never 0
    if (LDS) {
      uint32_t h = (key * 2654435761u) >> 19;                 // 13 bits: NUC_LDS_SLOTS, at most a quarter of them taken
      for (;;) {
        uint32_t cur = S.glcm[h];
        if (cur == 0u) {
          const uint32_t old = atomicCAS(&S.glcm[h], 0u, (key << 16) | 1u);
          if (old == 0u) break;
          cur = old;
        }
        if ((cur >> 16) == key) {
          atomicAdd(&S.glcm[h], 1u);                           // counts stay < 2^16 (at most NUC_LDS_PIXELS pairs)
          break;
        }
        h = (h + 1) & (NUC_LDS_SLOTS - 1);
      }
    } else {
      atomicAdd(&S.glcm[key], 1u);
    }
  }
  __syncthreads();
  long long sq = 0;
  for (int i = tid; i < nslots; i += NUC_THREADS) {
    const long long c = LDS ? (long long)(S.glcm[i] & 0xFFFFu) : (long long)S.glcm[i];
    sq += c * c;
  }
  nbg = block_sum(nbg, sh);
  sbg = block_sum(sbg, sh);
  ent = block_sum(ent, sh);
  npair = block_sum(npair, sh);
  sdis = block_sum(sdis, sh);
  sq = block_sum(sq, sh);

  // (c) components (8-connected foreground) and the outside background (4-connected), relaxed to their fixed point
  for (;;) {
    int changed = 0;
    for (int64_t p = tid; p < P; p += NUC_THREADS) {
      const int y = (int)(p / cw), x = (int)(p - (int64_t)y * cw);
      if (S.fg[p]) {
        int m = S.comp[p];
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const int yy = y + dy, xx = x + dx;
            if (yy < 0 || yy >= ch || xx < 0 || xx >= cw) continue;
            const int64_t q = (int64_t)yy * cw + xx;
            if (S.fg[q]) m = min(m, S.comp[q]);
          }
        if (m < S.comp[p]) {
          S.comp[p] = m;
          changed = 1;
        }
      } else if (!S.outer[p]) {
        if ((y > 0 && S.outer[p - cw]) || (y + 1 < ch && S.outer[p + cw]) || (x > 0 && S.outer[p - 1]) ||
            (x + 1 < cw && S.outer[p + 1])) {
          S.outer[p] = 1;
          changed = 1;
        }
      }
    }
    if (!__syncthreads_or(changed)) break;
  }
  // the chosen contour: the top-level component (left of its raster-first pixel: outside background) that starts LAST
  long long cand = -1;
  for (int64_t p = tid; p < P; p += NUC_THREADS) {
    const int x = (int)(p % cw);
    if (S.fg[p] && S.comp[p] == (int)p && (x == 0 || S.outer[p - 1])) cand = p;
  }
  const long long start = block_max(cand, sh);

  // (d) one lane: border following, CHAIN_APPROX_SIMPLE vertices, shoelace, hull, arc length, ellipse fit, moments
  if (tid == 0) {
    const int dxs[8] = {1, 1, 0, -1, -1, -1, 0, 1};         // OpenCV chain codes (y grows downwards)
    const int dys[8] = {0, -1, -1, -1, 0, 1, 1, 1};
    const int y0 = (int)(start / cw), x0 = (int)(start - (int64_t)y0 * cw);
    auto isfg = [&](int y, int x) { return y >= 0 && y < ch && x >= 0 && x < cw && S.fg[(int64_t)y * cw + x] != 0; };
    int64_t nv = 0;
    int overflow = 0;
    auto put = [&](int y, int x) {
      if (nv < S.vcap) S.verts[nv] = y * cw + x;
      else overflow = 1;
      ++nv;
    };
    int s = 4;
    do {
      s = (s - 1) & 7;
    } while (!isfg(y0 + dys[s], x0 + dxs[s]) && s != 4);
    if (s == 4) {
      put(y0, x0);                                            // a single pixel
    } else {
      const int y1 = y0 + dys[s], x1 = x0 + dxs[s];
      int y3 = y0, x3 = x0, prev_s = s ^ 4;
      const int64_t max_steps = 4 * P + 8;                    // a pixel lies at most 4 times on one border
      for (int64_t step = 0;; ++step) {
        if (step == max_steps) {
          overflow = 1;
          break;
        }
        int y4 = y3, x4 = x3;
        while (s < 15) {
          ++s;
          y4 = y3 + dys[s & 7];
          x4 = x3 + dxs[s & 7];
          if (isfg(y4, x4)) break;
        }
        s &= 7;
        if (s != prev_s) {
          put(y3, x3);
          prev_s = s;
        }
        if (y4 == y0 && x4 == x0 && y3 == y1 && x3 == x1) break;
        y3 = y4;
        x3 = x4;
        s = (s + 4) & 7;
      }
    }
    if (nv > S.vcap) nv = S.vcap;
    const int V = (int)nv;
    auto vx = [&](int i) { return (long long)(S.verts[i] % cw); };
    auto vy = [&](int i) { return (long long)(S.verts[i] / cw); };
    // contourArea and arcLength(closed): both walks start at the closing edge (last -> first); edge lengths are float sqrt
    long long a2 = 0;
    double perim = 0.0;
    if (V >= 2) {
      long long px = vx(V - 1), py = vy(V - 1);
      for (int i = 0; i < V; ++i) {
        const long long qx = vx(i), qy = vy(i);
        a2 += px * qy - py * qx;
        const float fdx = (float)(qx - px), fdy = (float)(qy - py);
        perim += (double)sqrtf(fdx * fdx + fdy * fdy);
        px = qx;
        py = qy;
      }
    }
    const double area = V >= 3 ? fabs((double)a2) * 0.5 : 0.0;
    // convex hull of the vertices (gift wrapping in exact integers; of collinear candidates the farthest)
    double hull_area = 0.0;
    if (V >= 3) {
      int st = 0;
      for (int i = 1; i < V; ++i)
        if (vx(i) < vx(st) || (vx(i) == vx(st) && vy(i) < vy(st))) st = i;
      long long h2 = 0;
      int cur = st;
      for (int it = 0; it <= V; ++it) {
        const long long cx = vx(cur), cy = vy(cur);
        int nx = -1;
        for (int q = 0; q < V; ++q) {
          const long long qx = vx(q) - cx, qy = vy(q) - cy;
          if (qx == 0 && qy == 0) continue;
          if (nx < 0) {
            nx = q;
            continue;
          }
          const long long bx = vx(nx) - cx, by = vy(nx) - cy;
          const long long cr = bx * qy - by * qx;
          if (cr < 0 || (cr == 0 && qx * qx + qy * qy > bx * bx + by * by)) nx = q;
        }
        if (nx < 0) break;
        h2 += cx * vy(nx) - cy * vx(nx);
        cur = nx;
        if (vx(cur) == vx(st) && vy(cur) == vy(st)) break;
      }
      hull_area = fabs((double)h2) * 0.5;
    }
    if (hull_area == 0.0) hull_area = 1.0;
    float fmaj = 1.f, fmin = 1.f, fang = 0.f;
    if (V > 4) {
      // fitEllipse (OpenCV 4.1 fitEllipseNoDirect) on the vertices centred on their mean and scaled into [-1, 1]
      long long sx = 0, sy = 0;
      for (int i = 0; i < V; ++i) {
        sx += vx(i);
        sy += vy(i);
      }
      const double mx = (double)sx / V, my = (double)sy / V;
      double amax = 0.0;
      for (int i = 0; i < V; ++i) amax = fmax(amax, fmax(fabs((double)vx(i) - mx), fabs((double)vy(i) - my)));
      const double sc = amax > 0.0 ? 1.0 / amax : 1.0;
      double G[25] = {0}, rhs[5] = {0}, g[5];
      for (int i = 0; i < V; ++i) {
        const double u = ((double)vx(i) - mx) * sc, v = ((double)vy(i) - my) * sc;
        const double a5[5] = {-u * u, -v * v, -u * v, u, v};
        for (int a = 0; a < 5; ++a) {
          rhs[a] += a5[a];
          for (int b = 0; b < 5; ++b) G[a * 5 + b] += a5[a] * a5[b];
        }
      }
      pinv_solve(G, rhs, g, 5, 1e-12);                        // singular values below 1e-6 of the largest dropped
      double M2[4] = {2 * g[0], g[2], g[2], 2 * g[1]}, b2[2] = {g[3], g[4]}, cc[2];
      pinv_solve(M2, b2, cc, 2, 1e-6);
      double G3[9] = {0}, r3[3] = {0}, h[3];
      for (int i = 0; i < V; ++i) {
        const double u = ((double)vx(i) - mx) * sc - cc[0], v = ((double)vy(i) - my) * sc - cc[1];
        const double a3[3] = {u * u, v * v, u * v};
        for (int a = 0; a < 3; ++a) {
          r3[a] += a3[a];
          for (int b = 0; b < 3; ++b) G3[a * 3 + b] += a3[a] * a3[b];
        }
      }
      pinv_solve(G3, r3, h, 3, 1e-12);
      for (int a = 0; a < 3; ++a) h[a] *= sc * sc;             // back to pixel units, where OpenCV's 1e-8 tests apply
      const double th = -0.5 * atan2(h[2], h[1] - h[0]);
      const double tt = fabs(h[2]) > 1e-8 ? h[2] / sin(-2.0 * th) : h[1] - h[0];
      double ra = fabs(h[0] + h[1] - tt), rb = fabs(h[0] + h[1] + tt);
      if (ra > 1e-8) ra = sqrt(2.0 / ra);
      if (rb > 1e-8) rb = sqrt(2.0 / rb);
      float bw = (float)(ra * 2), bh = (float)(rb * 2);
      if (bw > bh) {
        const float tmp = bw;
        bw = bh;
        bh = tmp;
        fang = (float)(90 + th * 180 / 3.14159265358979323846);
      }
      fmaj = fmaxf(bw, bh);
      fmin = fminf(bw, bh);
    }
    const double q = (double)fmin / (double)fmaj;
    const double ecc = fmaj != 0.f ? sqrt(1.0 - q * q) : 0.0;

    // intensity moments from the exact histogram, bins in ascending order
    long long nfg = 0, s1 = 0;
    for (int v = 0; v < 256; ++v) {
      nfg += sh.hist[v];
      s1 += (long long)sh.hist[v] * v;
    }
    const double mean = (double)s1 / (double)nfg;
    double m2 = 0.0, m3 = 0.0;
    for (int v = 0; v < 256; ++v) {
      if (!sh.hist[v]) continue;
      const double d = (double)v - mean;
      m2 += sh.hist[v] * (d * d);
      m3 += sh.hist[v] * (d * d * d);
    }
    m2 /= (double)nfg;
    m3 /= (double)nfg;
    const double skew = m2 == 0.0 ? 0.0 : m3 / pow(m2, 1.5);
    const double mean_fg = (double)s1 / ((double)nfg + 1e-8);
    const double mean_bg = (double)sbg / ((double)nbg + 1e-8);
    const double T = npair > 0 ? (double)npair : 1.0;
    double hom = 0.0;
    for (int d = 0; d < 256; ++d)
      if (sh.histd[d]) hom += (double)sh.histd[d] / (1.0 + (double)d * d);
    const double asmv = (double)sq / (T * T);

    float* o = feat + (int64_t)row * 16;
    o[0] = (float)mean_fg;
    o[1] = (float)fabs(mean_fg - mean_bg);
    o[2] = (float)m2;
    o[3] = (float)skew;
    o[4] = (float)(ent / (double)nfg);
    o[5] = (float)((double)sdis / T);
    o[6] = (float)(hom / T);
    o[7] = (float)sqrt(asmv);
    o[8] = (float)asmv;
    o[9] = (float)ecc;
    o[10] = (float)area;
    o[11] = fmaj;
    o[12] = fmin;
    o[13] = (float)perim;
    o[14] = (float)(area / hull_area);
    o[15] = fang;
    const double n = (double)t.cnt[L];
    cen[(int64_t)row * 2] = (float)((double)t.sr[L] / n);
    cen[(int64_t)row * 2 + 1] = (float)((double)t.sc[L] / n);
    if (info != nullptr) {
      info[(int64_t)row * 4] = y0;
      info[(int64_t)row * 4 + 1] = x0;
      info[(int64_t)row * 4 + 2] = overflow ? -V : V;
      info[(int64_t)row * 4 + 3] = LDS ? 0 : 1;
    }
  }
}

__global__ void __launch_bounds__(NUC_THREADS) k_nuc_lds(const int* __restrict__ labels, const uint8_t* __restrict__ gray, int H, int W,
                                                       int min_size, LabelTables t, const int* __restrict__ kept, float* feat, float* cen,
                                                       int* info) {
  __shared__ int comp[NUC_LDS_PIXELS];
  __shared__ uint8_t fg[NUC_LDS_PIXELS], outer[NUC_LDS_PIXELS];
  __shared__ uint32_t glcm[NUC_LDS_SLOTS];
  __shared__ Red sh;
  const int row = blockIdx.x;
  const int L = kept[row];
  if (crop_pixels(t, L, H, W) > NUC_LDS_PIXELS) return;      // listed for k_nuc_global
  Scratch S;
  S.comp = comp;
  S.fg = fg;
  S.outer = outer;
  S.glcm = glcm;
  S.verts = reinterpret_cast<int*>(glcm);                      // the hash is reduced before the contour is traced
  S.vcap = NUC_LDS_SLOTS;
  nucleus<true>(labels, gray, H, W, min_size, t, L, row, S, sh, feat, cen, info);
}

__host__ __device__ inline int64_t slot_bytes(int64_t max_px) {
  return align256(4 * max_px) + 2 * align256(max_px) + align256(4 * 65536) + align256(4 * (4 * max_px + 8));
}

__global__ void __launch_bounds__(NUC_THREADS) k_nuc_global(const int* __restrict__ labels, const uint8_t* __restrict__ gray, int H, int W,
                                                          int min_size, LabelTables t, const int* __restrict__ kept, int nbig, int64_t max_px,
                                                          char* big_ws, float* feat, float* cen, int* info) {
  __shared__ Red sh;
  char* base = big_ws + (int64_t)blockIdx.x * slot_bytes(max_px);
  Scratch S;
  S.comp = reinterpret_cast<int*>(base);
  base += align256(4 * max_px);
  S.fg = reinterpret_cast<uint8_t*>(base);
  base += align256(max_px);
  S.outer = reinterpret_cast<uint8_t*>(base);
  base += align256(max_px);
  S.glcm = reinterpret_cast<uint32_t*>(base);
  base += align256(4 * 65536);
  S.verts = reinterpret_cast<int*>(base);
  S.vcap = 4 * max_px + 8;
  for (int j = blockIdx.x; j < nbig; j += gridDim.x) {
    const int row = t.big_rows[j];
    nucleus<false>(labels, gray, H, W, min_size, t, kept[row], row, S, sh, feat, cen, info);
    __syncthreads();
  }
}

__global__ void k_bgr_to_gray(const uint8_t* __restrict__ bgr, int64_t npix, uint8_t* __restrict__ gray) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    const int b = bgr[3 * i], g = bgr[3 * i + 1], r = bgr[3 * i + 2];
    gray[i] = (uint8_t)((1868 * b + 9617 * g + 4899 * r + 8192) >> 14);
  }
}

}  // namespace

extern "C" int cgc_nuclei_lds_max_pixels(void) { return NUC_LDS_PIXELS; }

extern "C" int64_t cgc_nuclei_ws_bytes(int max_label) { return max_label < 0 ? 0 : layout_bytes(tables_layout, max_label); }

extern "C" int cgc_nuclei_label_pass(const int* labels, int H, int W, int max_label, int min_size, void* ws, int* kept_labels, int* meta,
                                     cgc_stream_t stream) {
  if (bad_image_dims(H, W) || max_label < 0 || ws == nullptr || meta == nullptr || (max_label > 0 && kept_labels == nullptr)) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const LabelTables t = tables_layout(Carver(ws), max_label);
  const int64_t ib = ceil_div64((int64_t)max_label + 1, 256);
  hipLaunchKernelGGL(k_nuc_init, dim3((int)(ib < 1024 ? ib : 1024)), dim3(256), 0, st, t, meta);
  CGC_RETURN_IF_LAUNCH_FAILED();
  const int64_t npix = (int64_t)H * W;
  if (npix > 0) {
    const int64_t nb = ceil_div64(npix, 256);
    hipLaunchKernelGGL(k_nuc_label_pass, dim3((int)(nb < 8192 ? nb : 8192)), dim3(256), 0, st, labels, H, W, t, meta);
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  hipLaunchKernelGGL(k_nuc_compact, dim3(1), dim3(1024), 0, st, t, H, W, min_size, kept_labels, meta);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}

extern "C" int64_t cgc_nuclei_big_ws_bytes(int nbig, int64_t max_big_px) {
  if (nbig <= 0 || max_big_px <= 0) return 0;
  const int slots = nbig < NUC_BIG_SLOTS ? nbig : NUC_BIG_SLOTS;
  return slots * slot_bytes(max_big_px);
}

extern "C" int cgc_nuclei_features(const int* labels, const uint8_t* gray, int H, int W, int max_label, int min_size, const void* ws,
                                   const int* kept_labels, int n, int nbig, int64_t max_big_px, void* big_ws, float* features,
                                   float* centroids, int* info, cgc_stream_t stream) {
  if (bad_image_dims(H, W) || max_label < 0 || n < 0 || nbig < 0 || nbig > n || ws == nullptr) return CGC_EINVAL;
  if (n == 0) return 0;
  if (nbig > 0 && (big_ws == nullptr || max_big_px <= NUC_LDS_PIXELS || max_big_px > (int64_t)H * W)) return CGC_EINVAL;
  hipStream_t st = as_stream(stream);
  const LabelTables t = tables_layout(Carver(const_cast<void*>(ws)), max_label);
  hipLaunchKernelGGL(k_nuc_lds, dim3(n), dim3(NUC_THREADS), 0, st, labels, gray, H, W, min_size, t, kept_labels, features, centroids, info);
  CGC_RETURN_IF_LAUNCH_FAILED();
  if (nbig > 0) {
    const int slots = nbig < NUC_BIG_SLOTS ? nbig : NUC_BIG_SLOTS;
    hipLaunchKernelGGL(k_nuc_global, dim3(slots), dim3(NUC_THREADS), 0, st, labels, gray, H, W, min_size, t, kept_labels, nbig, max_big_px,
                       static_cast<char*>(big_ws), features, centroids, info);
    CGC_RETURN_IF_LAUNCH_FAILED();
  }
  return 0;
}

extern "C" int cgc_bgr_to_gray(const uint8_t* bgr, int64_t npix, uint8_t* gray, cgc_stream_t stream) {
  if (npix < 0) return CGC_EINVAL;
  if (npix == 0) return 0;
  const int64_t nb = ceil_div64(npix, 256);
  hipLaunchKernelGGL(k_bgr_to_gray, dim3((int)(nb < 4096 ? nb : 4096)), dim3(256), 0, as_stream(stream), bgr, npix, gray);
  CGC_RETURN_IF_LAUNCH_FAILED();
  return 0;
}
