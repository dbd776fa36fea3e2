// Device-side surface voxelisation of STL meshes (tclb_amd/geometry/stl.py draw_stl,
// side="surface"): the sub-voxel cut distances of the 26 D3Q27 links and the surface mask,
// bit-identical to the host voxeliser (csrc/runtime/host.cpp tclb_stl_cuts).
//
//   k_tri_prep    one lane per triangle: integer bounding box clipped to the window and its
//                 number of 256-node chunks (scanned by hipcub into chunk offsets)
//   k_stl_cuts    one work-group per chunk, one wave per 64 nodes of it: cut distances of one
//                 triangle at those nodes, min-scattered into the window array
//   k_cuts_merge  unsigned min of a window array into the lattice's cut array through the
//                 local -> global row tables (ghost and periodic-wrap rows get their copies)
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

// lane t: box and chunk count of triangle t; lane ntri: the closing 0 whose scan is the total
__global__ void __launch_bounds__(256) k_tri_prep(const double* __restrict__ tri, int ntri, Window w,
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

bool window_ok(const Window& w) { return w.wx >= 0 && w.wy >= 0 && w.wz >= 0; }

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
  const Window w = {x0, y0, z0, wx, wy, wz};
  VoxTmp t;
  if (ntri < 0 || !window_ok(w) || !nchunks) return (int)hipErrorInvalidValue;
  *nchunks = 0;
  if (ntri == 0) return 0;
  if (!tri || !vox_tmp(tmp, tmp_bytes, ntri, t)) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  k_tri_prep<<<dim3((unsigned)(ntri / 256 + 1)), dim3(256), 0, s>>>((const double*)tri, ntri, w, t.box, t.cnt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  size_t tb = t.temp_bytes;
  if ((e = hipcub::DeviceScan::ExclusiveSum(t.temp, tb, t.cnt, t.off, ntri + 1, s)) != hipSuccess) return (int)e;
  if ((e = hipMemcpyAsync(nchunks, t.off + ntri, sizeof(long long), hipMemcpyDeviceToHost, s)) != hipSuccess)
    return (int)e;
  return (int)hipStreamSynchronize(s);
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
