// Device-side voxelisation of STL meshes (tclb_amd/geometry/stl.py draw_stl): for
// side="surface" the sub-voxel cut distances of the 26 D3Q27 links and the surface mask, for
// side="in" / "out" the ray-parity levels of a solid body, both bit-identical to the host
// voxeliser (csrc/runtime/host.cpp tclb_stl_cuts, tclb_stl_fill).
//
//   k_tri_prep    one lane per triangle: integer bounding box clipped to the window and its
//                 number of 256-node chunks (scanned by hipcub into chunk offsets); for the
//                 fill the box is flat, one cell thick along the ray axis
//   k_stl_cuts    one work-group per chunk, one wave per 64 nodes of it: cut distances of one
//                 triangle at those nodes, min-scattered into the window array
//   k_cuts_merge  unsigned min of a window array into the lattice's cut array through the
//                 local -> global row tables (ghost and periodic-wrap rows get their copies)
//   k_stl_hits    one work-group per chunk of a triangle's clipped rectangle across the ray
//                 axis, one wave per 64 ray columns: barycentric test of the column, height h
//                 of the hit, +1 on the uint32 counter at (column, min(floor(h), window top))
//   k_ray_rows    ray axis y or z: a lane owns one x, a wave 64 consecutive x of one row of
//                 columns; it marches down the ray with the running sum in a register, every
//                 load and store a coalesced 64-wide row
//   k_ray_x       ray axis x: a wave owns one column and walks it 64 cells a trip from the
//                 top, an inclusive cross-lane scan per trip and a carry between trips
//
// Fill: the host increments a byte at every node from the region bottom up to floor(h) for
// every hit, so lev[x1] = (inside_out + #{hits of the column with floor(h) >= x1}) mod 256: a
// scatter of hit tops and a suffix sum along the ray.  The counters are 32 bits wide, so any
// number of hits below 2^32 on one cell wraps exactly as the host's byte does, and integer
// addition commutes, so the scatter is deterministic.  Counters exist from the mesh's lowest
// box cell (ceil(min) - 1) upwards only; below it the sum is constant and the scan kernels
// fill down to the region bottom without reading.  k_stl_hits performs tclb_stl_fill's
// operations one for one: v1, v2, c0, dc1-3 per triangle (wave-uniform), c1, c2,
// c3 = 1. - c1 - c2, the topo rule with its c == 0 ties and h per lane.
//
// Bit equality: the host library is plain IEEE fp64 without fused multiply-adds, so contraction
// is off for this whole file and k_stl_cuts performs the operations of gauss4 / calc_cut one
// for one, in their order.  Min is order independent, so the scatter is deterministic.
//
// k_stl_cuts, work split: triangle-major.  The lanes of a chunk enumerate the nodes of the
// triangle's clipped box x fastest, so the 3^3-4^3 boxes of a fine mesh fill a wave and a large
// triangle spreads over many work-groups.  The triangle of a chunk is found by a binary search
// over the scanned offsets; the search, the nine coordinates, the box and the direction table
// depend on the block index only, i.e. they are wave-uniform scalar loads held in SGPRs.
//
// k_stl_cuts, shared elimination: the host solves a fresh 4 x 4 system per (node, direction),
// but only column 3 of it (the direction) and nothing else depends on the direction: pivot
// tests, row swaps and multipliers of the elimination read columns 0-2 alone.  A lane
// therefore eliminates columns 0-2 and the right-hand side once, keeps the three swap rows
// and six multipliers in registers, and per direction replays the column-3 updates
// A[i][3] -= m * A[k][3] and the back substitution: 6 + 26 * (1 to 4) divisions per node
// instead of 26 * 10, every single operation the host's.
//
// The window array is (26, plane) uint16 with plane = wz * wy * wx rounded up to even, so each
// direction starts on a dword: the 16-bit min is a compare-and-swap loop on the aligned dword
// that holds the half.
//
// Every launcher returns 0 or a HIP error code and takes its stream explicitly.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <math.h>

#include <cstdint>

#include <hipcub/hipcub.hpp>

namespace {

constexpr int VOX_BLOCK = 256;   // nodes per chunk: 4 waves of 64
constexpr int NDIRS = 26;

struct Window { int x0, y0, z0, wx, wy, wz; };

// scratch of one voxelisation: chunk counts and offsets (ntri + 1 each), boxes (lo xyz, n xyz),
// the scan's temporary storage; every part aligned to 256 bytes
struct VoxTmp {
  long long *cnt, *off;
  int* box;
  void* temp;
  size_t temp_bytes;
};

size_t align256(size_t b) { return (b + 255) / 256 * 256; }

size_t scan_temp_bytes(int ntri) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (long long*)nullptr, (long long*)nullptr, ntri + 1);
  return b;
}

size_t vox_tmp_bytes(int ntri) {
  return 2 * align256(sizeof(long long) * ((size_t)ntri + 1)) + align256(sizeof(int) * 6 * (size_t)(ntri > 0 ? ntri : 1)) +
         align256(scan_temp_bytes(ntri));
}

bool vox_tmp(void* tmp, long long bytes, int ntri, VoxTmp& t) {
  if (!tmp || ((uintptr_t)tmp & 255u) || bytes < (long long)vox_tmp_bytes(ntri)) return false;
  char* p = (char*)tmp;
  const size_t nl = align256(sizeof(long long) * ((size_t)ntri + 1));
  t.cnt = (long long*)p, p += nl;
  t.off = (long long*)p, p += nl;
  t.box = (int*)p, p += align256(sizeof(int) * 6 * (size_t)(ntri > 0 ? ntri : 1));
  t.temp = p;
  t.temp_bytes = scan_temp_bytes(ntri);
  return true;
}

// lane t: box and chunk count of triangle t; lane ntri: the closing 0 whose scan is the total.
// flat = 0, 1, 2: the box is the window's first cell along that axis whatever the triangle's
// extent there (the rectangle of ray columns of the fill); -1: the full box
__global__ void __launch_bounds__(256) k_tri_prep(const double* __restrict__ tri, int ntri, Window w, int flat,
                                                  int* __restrict__ box, long long* __restrict__ cnt) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t > ntri) return;
  if (t == ntri) {
    cnt[t] = 0;
    return;
  }
  const double* p = tri + 9 * (long long)t;
  const int w0[3] = {w.x0, w.y0, w.z0}, wn[3] = {w.wx, w.wy, w.wz};
  long long nodes = 1;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const double a = fmin(p[j], fmin(p[3 + j], p[6 + j]));
    const double b = fmax(p[j], fmax(p[3 + j], p[6 + j]));
    long long lo = (long long)(int)ceil(a) - 1, hi = (long long)(int)floor(b) + 1;
    if (lo < w0[j]) lo = w0[j];
    if (hi > (long long)w0[j] + wn[j] - 1) hi = (long long)w0[j] + wn[j] - 1;
    if (j == flat) lo = hi = w0[j];
    const long long n = hi >= lo ? hi - lo + 1 : 0;
    box[6 * (long long)t + j] = (int)lo;
    box[6 * (long long)t + 3 + j] = (int)n;
    nodes *= n;
  }
  cnt[t] = (nodes + VOX_BLOCK - 1) / VOX_BLOCK;
}

// unsigned 16-bit min of v into half `idx` of the dword array h
__device__ __forceinline__ void min_u16(uint32_t* __restrict__ h, long long idx, uint32_t v) {
  uint32_t* wd = h + (idx >> 1);
  const uint32_t sh = (uint32_t)(idx & 1) * 16u;
  uint32_t old = __atomic_load_n(wd, __ATOMIC_RELAXED);
  while (v < ((old >> sh) & 0xffffu)) {
    const uint32_t want = (old & ~(0xffffu << sh)) | (v << sh);
    const uint32_t prev = atomicCAS(wd, old, want);
    if (prev == old) break;
    old = prev;
  }
}

__device__ __forceinline__ void swap_if(bool c, double& a, double& b) {
  const double ta = a, tb = b;
  a = c ? tb : ta;
  b = c ? ta : tb;
}

// cuts: (26, plane) uint16 as dwords, all 0xFFFF before; mask: (wz, wy, wx) bytes, 0 before
__global__ void __launch_bounds__(VOX_BLOCK) k_stl_cuts(const double* __restrict__ tri, int ntri,
                                                        const long long* __restrict__ off,
                                                        const int* __restrict__ box, const int* __restrict__ dirs,
                                                        Window w, long long plane, uint32_t* __restrict__ cuts,
                                                        unsigned char* __restrict__ mask) {
  // the triangle of this chunk: off[t] <= chunk < off[t + 1] (triangles without chunks have
  // off[t] == off[t + 1] and are never found); off[0] = 0, off[ntri] = number of chunks
  const long long chunk = blockIdx.x;
  int t = 0, hi = ntri;
  while (hi - t > 1) {
    const int mid = (t + hi) >> 1;
    if (off[mid] <= chunk) t = mid; else hi = mid;
  }
  const int* bx = box + 6 * (long long)t;
  const int bnx = bx[3], bny = bx[4], bnz = bx[5];
  const long long n = (chunk - off[t]) * VOX_BLOCK + threadIdx.x;
  if (n >= (long long)bnx * bny * bnz) return;
  const long long row = n / bnx;
  const int gx = bx[0] + (int)(n - row * bnx);
  const int gy = bx[1] + (int)(row % bny);
  const int gz = bx[2] + (int)(row / bny);

  // columns 0-2 and right-hand side of calc_cut's system: X - p1, X - p2, X - p3 | 1 1 1
  const double* p = tri + 9 * (long long)t;
  const double X[3] = {(double)gx, (double)gy, (double)gz};
  double a[4][3], b[4] = {0, 0, 0, 1};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    a[i][0] = X[i] - p[i];
    a[i][1] = X[i] - p[3 + i];
    a[i][2] = X[i] - p[6 + i];
  }
  a[3][0] = a[3][1] = a[3][2] = 1;

  // gauss4's elimination without column 3; sw[k]: the row swapped with k (0: none, a swap
  // partner is never row 0), m[k][i]: the multiplier of row i in step k.  The entries below
  // the diagonal are never read again and are not formed.
  int sw[3];
  double m[3][4];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    int s = 0;
    if (fabs(a[k][k]) < 1e-10) {
#pragma unroll
      for (int i = k + 1; i < 4; i++)
        if (s == 0 && fabs(a[i][k]) >= 1e-10) s = i;
    }
#pragma unroll
    for (int i = k + 1; i < 4; i++) {
#pragma unroll
      for (int j = 0; j < 3; j++) swap_if(s == i, a[k][j], a[i][j]);
      swap_if(s == i, b[k], b[i]);
    }
    sw[k] = s;
#pragma unroll
    for (int i = k + 1; i < 4; i++) {
      const double mm = a[i][k] / a[k][k];
      m[k][i] = mm;
#pragma unroll
      for (int j = k + 1; j < 3; j++) a[i][j] -= mm * a[k][j];
      b[i] -= mm * b[k];
    }
  }

  const long long node = (gx - w.x0) + (long long)w.wx * ((gy - w.y0) + (long long)w.wy * (gz - w.z0));
  bool any = false;
  for (int d = 0; d < NDIRS; d++) {
    // column 3 through the recorded swaps and multipliers
    double c[4] = {(double)dirs[3 * d], (double)dirs[3 * d + 1], (double)dirs[3 * d + 2], 0};
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
      for (int i = k + 1; i < 4; i++) swap_if(sw[k] == i, c[k], c[i]);
#pragma unroll
      for (int i = k + 1; i < 4; i++) c[i] -= m[k][i] * c[k];
    }
    // back substitution, sums started at 0 and taken left to right as on the host; a failed
    // r3 rejects the direction whatever the others are
    double s = 0;
    const double r3 = (b[3] - s) / c[3];
    if (!(r3 >= 0) || r3 > 1) continue;
    s = 0;
    s += c[2] * r3;
    const double r2 = (b[2] - s) / a[2][2];
    s = 0;
    s += a[1][2] * r2;
    s += c[1] * r3;
    const double r1 = (b[1] - s) / a[1][1];
    s = 0;
    s += a[0][1] * r1;
    s += a[0][2] * r2;
    s += c[0] * r3;
    const double r0 = (b[0] - s) / a[0][0];
    if (!(r0 >= 0) || !(r1 >= 0) || !(r2 >= 0)) continue;
    const uint32_t q = (uint32_t)(uint16_t)(int)(r3 * 65000.0);
    min_u16(cuts, (long long)d * plane + node, q);
    any = true;
  }
  if (any) mask[node] = 1;
}

// block (row, x-run, direction): local row `row` = k * NY + j of dst lies at global (ys[j], zs[k])
__global__ void __launch_bounds__(VOX_BLOCK) k_cuts_merge(uint16_t* __restrict__ dst, int NY, int px,
                                                          long long dplane, const uint16_t* __restrict__ win,
                                                          long long plane, Window w, const int* __restrict__ ys,
                                                          const int* __restrict__ zs) {
  const int k = blockIdx.x / NY, j = blockIdx.x - k * NY;
  const int Y = ys[j] - w.y0, Z = zs[k] - w.z0;
  if (Y < 0 || Y >= w.wy || Z < 0 || Z >= w.wz) return;
  const int x = blockIdx.y * VOX_BLOCK + threadIdx.x;
  if (x >= w.wx) return;
  const int d = blockIdx.z;
  const uint16_t v = win[d * plane + x + (long long)w.wx * (Y + (long long)w.wy * Z)];
  uint16_t* o = dst + d * dplane + (long long)blockIdx.x * px + w.x0 + x;
  if (v < *o) *o = v;
}

// topo term of one barycentric coordinate: positive, or zero with a positive tie-breaker
__device__ __forceinline__ int topo1(double c, double dc) { return c == 0 ? (dc > 0 ? 1 : 0) : (c > 0 ? 1 : 0); }

__device__ __forceinline__ int pick3(int a, int b, int c, int i) { return i == 0 ? a : (i == 1 ? b : c); }

// cnt: uint32 counters over the window with the ray axis cut down to [cb, cb + cn), x fastest,
// all 0 before; box: flat boxes of k_tri_prep(flat = axis)
__global__ void __launch_bounds__(VOX_BLOCK) k_stl_hits(const double* __restrict__ tri, int ntri,
                                                        const long long* __restrict__ off,
                                                        const int* __restrict__ box, Window w, int axis, int cb,
                                                        int cn, uint32_t* __restrict__ cnt) {
  const long long chunk = blockIdx.x;
  int t = 0, hi = ntri;
  while (hi - t > 1) {
    const int mid = (t + hi) >> 1;
    if (off[mid] <= chunk) t = mid; else hi = mid;
  }
  // per triangle, wave-uniform: tclb_stl_fill's v1, v2, c0, dc1, dc2, dc3
  const int ax1 = axis, ax2 = (axis + 1) % 3, ax3 = (axis + 2) % 3;
  const double *p1 = tri + 9 * (long long)t, *p2 = p1 + 3, *p3 = p1 + 6;
  const double v10 = p2[ax2] - p1[ax2], v11 = p2[ax3] - p1[ax3];
  const double v20 = p3[ax2] - p1[ax2], v21 = p3[ax3] - p1[ax3];
  const double c0 = v10 * v21 - v11 * v20;
  if (c0 == 0) return;
  const double dv0 = -0.5694552, dv1 = 0.8220224;
  const double dc1 = (v10 * dv1 - v11 * dv0) / c0;
  const double dc2 = (dv0 * v21 - dv1 * v20) / c0;
  const double dc3 = -dc1 - dc2;

  const int* bx = box + 6 * (long long)t;
  const int bnx = bx[3], bny = bx[4], bnz = bx[5];
  const long long n = (chunk - off[t]) * VOX_BLOCK + threadIdx.x;
  if (n >= (long long)bnx * bny * bnz) return;
  const long long row = n / bnx;
  const int gx = bx[0] + (int)(n - row * bnx);
  const int gy = bx[1] + (int)(row % bny);
  const int gz = bx[2] + (int)(row / bny);

  // per column: c1, c2, c3, the three-way rule, the height of the hit
  const double u0 = pick3(gx, gy, gz, ax2) - p1[ax2], u1 = pick3(gx, gy, gz, ax3) - p1[ax3];
  const double c1 = (v10 * u1 - v11 * u0) / c0;
  const double c2 = (u0 * v21 - u1 * v20) / c0;
  const double c3 = 1. - c1 - c2;
  if (topo1(c1, dc1) + topo1(c2, dc2) + topo1(c3, dc3) != 3) return;
  const double h = p1[ax1] * c3 + p2[ax1] * c2 + p3[ax1] * c1;

  // the host's loop runs x1 = bottom ... while x1 <= h, inside the region only
  const int bot = pick3(w.x0, w.y0, w.z0, axis), top = bot + pick3(w.wx, w.wy, w.wz, axis) - 1;
  if (!((double)bot <= h)) return;
  int lv = (h >= (double)top ? top : (int)floor(h)) - cb;
  lv = lv < 0 ? 0 : (lv >= cn ? cn - 1 : lv);
  // the column lies in the window (its box is clipped to it), the level in [0, cn)
  const int X = axis == 0 ? lv : gx - w.x0, Y = axis == 1 ? lv : gy - w.y0, Z = axis == 2 ? lv : gz - w.z0;
  const int dx = axis == 0 ? cn : w.wx, dy = axis == 1 ? cn : w.wy;
  atomicAdd(cnt + (X + (long long)dx * (Y + (long long)dy * Z)), 1u);
}

// axis 1 or 2.  block (64 x, 4 rows of the other cross axis); lev (wz, wy, wx) bytes, written
// in full: (io + suffix sum of cnt from the window top) mod 256, constant below level cb
__global__ void __launch_bounds__(VOX_BLOCK) k_ray_rows(const uint32_t* __restrict__ cnt, Window w, int axis, int cb,
                                                        int cn, uint32_t io, unsigned char* __restrict__ lev) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int o = blockIdx.y * (VOX_BLOCK / 64) + (threadIdx.x >> 6);
  if (x >= w.wx || o >= (axis == 1 ? w.wz : w.wy)) return;
  const long long rowl = w.wx, planel = (long long)w.wx * w.wy;
  // strides along the ray and base of column (x, o), in lev and in cnt
  const long long ls = axis == 1 ? rowl : planel, cs = ls;
  const int nbelow = cb - (axis == 1 ? w.y0 : w.z0);
  unsigned char* l = lev + x + (axis == 1 ? planel * o : rowl * o);
  const uint32_t* c = cnt + x + (axis == 1 ? rowl * cn * o : rowl * o);
  uint32_t sum = io;
#pragma unroll 8
  for (int k = cn - 1; k >= 0; k--) {
    sum += c[k * cs];
    l[(k + nbelow) * ls] = (unsigned char)sum;
  }
  for (int k = nbelow - 1; k >= 0; k--) l[k * ls] = (unsigned char)sum;
}

// axis 0.  one wave per column (y, z), 4 columns per block; lane i of trip j holds the cell
// i + 64 j below the window top, so the suffix sum is an inclusive scan over the lanes
__global__ void __launch_bounds__(VOX_BLOCK) k_ray_x(const uint32_t* __restrict__ cnt, Window w, int cb, int cn,
                                                     uint32_t io, unsigned char* __restrict__ lev) {
  const long long col = (long long)blockIdx.x * (VOX_BLOCK / 64) + (threadIdx.x >> 6);
  if (col >= (long long)w.wy * w.wz) return;      // wave-uniform
  const int lane = threadIdx.x & 63, nbelow = cb - w.x0;
  const uint32_t* c = cnt + col * cn;
  unsigned char* l = lev + col * w.wx;
  uint32_t carry = io;
  for (int base = cn - 1; base >= 0; base -= 64) {
    const int k = base - lane;
    uint32_t v = k >= 0 ? c[k] : 0u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t u = __shfl_up(v, d);
      if (lane >= d) v += u;
    }
    v += carry;
    if (k >= 0) l[k + nbelow] = (unsigned char)v;
    carry = __shfl(v, 63);
  }
  for (int k = nbelow - 1 - lane; k >= 0; k -= 64) l[k] = (unsigned char)carry;
}

bool window_ok(const Window& w) { return w.wx >= 0 && w.wy >= 0 && w.wz >= 0; }

// boxes (flat along `flat`, or full for -1) and scanned chunk offsets into tmp; *nchunks: their
// total, valid on return (the stream is synchronised)
int prep(const void* tri, int ntri, const Window& w, int flat, void* tmp, long long tmp_bytes, long long* nchunks,
         void* stream) {
  VoxTmp t;
  if (ntri < 0 || !window_ok(w) || !nchunks) return (int)hipErrorInvalidValue;
  *nchunks = 0;
  if (ntri == 0) return 0;
  if (!tri || !vox_tmp(tmp, tmp_bytes, ntri, t)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  k_tri_prep<<<dim3((unsigned)(ntri / 256 + 1)), dim3(256), 0, s>>>((const double*)tri, ntri, w, flat, t.box, t.cnt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  size_t tb = t.temp_bytes;
  if ((e = hipcub::DeviceScan::ExclusiveSum(t.temp, tb, t.cnt, t.off, ntri + 1, s)) != hipSuccess) return (int)e;
  if ((e = hipMemcpyAsync(nchunks, t.off + ntri, sizeof(long long), hipMemcpyDeviceToHost, s)) != hipSuccess)
    return (int)e;
  return (int)hipStreamSynchronize(s);
}

}  // namespace

// bytes of the scratch buffer tclb_stl_prep and tclb_stl_cuts share for ntri triangles
extern "C" long long tclb_stl_tmp_bytes(int ntri) {
  if (ntri < 0) return -1;
  return (long long)vox_tmp_bytes(ntri);
}

// boxes and scanned chunk offsets of ntri triangles (tri: ntri x 9 doubles on the device) over
// the window into tmp (256-byte aligned, tclb_stl_tmp_bytes); *nchunks: their total, valid on
// return (the stream is synchronised)
extern "C" int tclb_stl_prep(const void* tri, int ntri, int x0, int y0, int z0, int wx, int wy, int wz, void* tmp,
                             long long tmp_bytes, long long* nchunks, void* stream) {
  return prep(tri, ntri, Window{x0, y0, z0, wx, wy, wz}, -1, tmp, tmp_bytes, nchunks, stream);
}

// the same for the fill along `axis`: the box of a triangle is its rectangle of ray columns
// clipped to the window, one cell thick
extern "C" int tclb_stl_prep_rays(const void* tri, int ntri, int x0, int y0, int z0, int wx, int wy, int wz,
                                  int axis, void* tmp, long long tmp_bytes, long long* nchunks, void* stream) {
  if (axis < 0 || axis > 2) return (int)hipErrorInvalidValue;
  const Window w = {x0, y0, z0, wx, wy, wz};
  if (window_ok(w) && nchunks && (long long)wx * wy * wz == 0) {
    *nchunks = 0;
    return 0;
  }
  return prep(tri, ntri, w, axis, tmp, tmp_bytes, nchunks, stream);
}

// ray-parity levels lev (wz * wy * wx bytes, written in full) of the window from the triangles
// prepared into tmp by tclb_stl_prep_rays with the same axis: inside_out + the number of hits
// at or above a node along `axis`, mod 256, what tclb_stl_fill of the host library leaves in
// these nodes.  The window starts at the region bottom along the ray; cb >= that bottom is the
// lowest level a hit's floor(h) can take (lower ones are counted at cb), and cnt holds the
// counters of the levels cb ... window top: cnt_bytes >= 4 * their number, 4-byte aligned,
// cleared here.
extern "C" int tclb_stl_ray_fill(const void* tri, int ntri, int x0, int y0, int z0, int wx, int wy, int wz, int axis,
                                 int inside_out, int cb, void* tmp, long long tmp_bytes, long long nchunks,
                                 void* cnt, long long cnt_bytes, void* lev, void* stream) {
  const Window w = {x0, y0, z0, wx, wy, wz};
  VoxTmp t;
  if (ntri < 0 || !window_ok(w) || nchunks < 0 || nchunks > 0x7fffffffLL || axis < 0 || axis > 2)
    return (int)hipErrorInvalidValue;
  const long long nodes = (long long)wx * wy * wz;
  if (nodes == 0) return 0;
  const int bot = axis == 0 ? x0 : (axis == 1 ? y0 : z0), nray = axis == 0 ? wx : (axis == 1 ? wy : wz);
  if (cb < bot || cb - bot >= nray) return (int)hipErrorInvalidValue;
  const int cn = bot + nray - cb;
  const long long cells = nodes / nray * cn;
  if (!cnt || !lev || ((uintptr_t)cnt & 3u)) return (int)hipErrorInvalidDevicePointer;
  if (cnt_bytes < 4 * cells) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(cnt, 0, (size_t)cells * sizeof(uint32_t), s);
  if (e != hipSuccess) return (int)e;
  if (ntri > 0 && nchunks > 0) {
    if (!tri || !vox_tmp(tmp, tmp_bytes, ntri, t)) return (int)hipErrorInvalidValue;
    k_stl_hits<<<dim3((unsigned)nchunks), dim3(VOX_BLOCK), 0, s>>>((const double*)tri, ntri, t.off, t.box, w, axis,
                                                                    cb, cn, (uint32_t*)cnt);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  }
  constexpr int W = VOX_BLOCK / 64;
  if (axis == 0) {
    const long long cols = (long long)wy * wz;
    k_ray_x<<<dim3((unsigned)((cols + W - 1) / W)), dim3(VOX_BLOCK), 0, s>>>((const uint32_t*)cnt, w, cb, cn,
                                                                             (uint32_t)inside_out,
                                                                             (unsigned char*)lev);
  } else {
    const int no = axis == 1 ? wz : wy;
    if ((no + W - 1) / W > 65535) return (int)hipErrorInvalidValue;
    k_ray_rows<<<dim3((unsigned)((wx + 63) / 64), (unsigned)((no + W - 1) / W)), dim3(VOX_BLOCK), 0, s>>>(
        (const uint32_t*)cnt, w, axis, cb, cn, (uint32_t)inside_out, (unsigned char*)lev);
  }
  return (int)hipGetLastError();
}

// cuts ((26, plane) uint16, 4-byte aligned, plane even and >= wx * wy * wz) and mask (wz * wy * wx
// bytes) of the window from the triangles prepared into tmp: both are cleared here (0xFFFF / 0),
// then the nchunks chunks tclb_stl_prep counted are worked off; dirs: 26 x 3 ints on the device
extern "C" int tclb_stl_cuts(const void* tri, int ntri, int x0, int y0, int z0, int wx, int wy, int wz,
                             const void* dirs, void* tmp, long long tmp_bytes, long long nchunks, void* cuts,
                             long long plane, void* mask, void* stream) {
  const Window w = {x0, y0, z0, wx, wy, wz};
  VoxTmp t;
  if (ntri < 0 || !window_ok(w) || nchunks < 0 || nchunks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  const long long nodes = (long long)wx * wy * wz;
  if (nodes == 0) return 0;
  if (!cuts || !mask || ((uintptr_t)cuts & 3u)) return (int)hipErrorInvalidDevicePointer;
  if (plane < nodes || (plane & 1)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(cuts, 0xFF, (size_t)plane * NDIRS * sizeof(uint16_t), s);
  if (e != hipSuccess) return (int)e;
  if ((e = hipMemsetAsync(mask, 0, (size_t)nodes, s)) != hipSuccess) return (int)e;
  if (ntri == 0 || nchunks == 0) return 0;
  if (!tri || !dirs || !vox_tmp(tmp, tmp_bytes, ntri, t)) return (int)hipErrorInvalidValue;
  k_stl_cuts<<<dim3((unsigned)nchunks), dim3(VOX_BLOCK), 0, s>>>((const double*)tri, ntri, t.off, t.box,
                                                                  (const int*)dirs, w, plane, (uint32_t*)cuts,
                                                                  (unsigned char*)mask);
  return (int)hipGetLastError();
}

// dst ((26, NZ, NY, px) uint16, direction stride dplane elements) = min(dst, win) where the
// local row (k, j) lies at global (ys[j], zs[k]) inside the window (x0, y0, z0, wx, wy, wz) of
// win ((26, plane) uint16, rows of wx); x is not decomposed: global x = local x < px
extern "C" int tclb_cuts_merge(void* dst, int NZ, int NY, int px, long long dplane, const void* win,
                               long long plane, int x0, int y0, int z0, int wx, int wy, int wz, const void* ys,
                               const void* zs, void* stream) {
  const Window w = {x0, y0, z0, wx, wy, wz};
  if (NZ < 0 || NY < 0 || px < 0 || !window_ok(w)) return (int)hipErrorInvalidValue;
  const long long rows = (long long)NZ * NY, nodes = (long long)wx * wy * wz;
  if (rows == 0 || nodes == 0) return 0;
  if (x0 < 0 || (long long)x0 + wx > px || dplane < rows * px || plane < nodes || rows > 0x7fffffffLL)
    return (int)hipErrorInvalidValue;
  if (!dst || !win || !ys || !zs) return (int)hipErrorInvalidDevicePointer;
  const dim3 grid((unsigned)rows, (unsigned)((wx + VOX_BLOCK - 1) / VOX_BLOCK), NDIRS);
  k_cuts_merge<<<grid, dim3(VOX_BLOCK), 0, (hipStream_t)stream>>>((uint16_t*)dst, NY, px, dplane,
                                                                   (const uint16_t*)win, plane, w, (const int*)ys,
                                                                   (const int*)zs);
  return (int)hipGetLastError();
}
