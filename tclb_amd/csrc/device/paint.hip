// Device-side geometry painting (tclb_amd/geometry/geometry.py Geometry, TCLB_GEOMETRY): the
// primitives of a <Geometry> element as a display list, rasterised into the rank's flag
// array by one kernel, bit-identical to the NumPy painter of the host path.
//
//   k_paint   flags (NZ, NY, gnx) uint32, local row (k, j) at global (ys[j], zs[k]) (ghost and
//             periodic-wrap rows repeat coordinates), records in drawing order.  Per node, for
//             every record in order: if the node's global (x, y, z) lies in the record's box
//             and its predicate holds, and the current value v passes the mode (overwrite:
//             always, fill: (v & mask) == 0, change: (v & mask) != 0), v = (v & ~mask) | fg.
//             A flag is loaded once and stored once for the whole list, and only if it changed.
//
// Work split: a wave is one 64-node x-segment of one row, so the y and z box tests and the
// row's Y / Z doubles are wave-uniform and only x is per lane.  A work-group of four waves owns
// a tile of TILE_X x TILE_Y rows x TILE_Z planes; wave w owns row w of the tile and marches its
// planes.
//
// Culling: before any flag is touched the work-group tests the records against its tile, 256
// records a round, one record per lane: the box against the tile's x range and against the
// tile's sets of global y and z coordinates (sets, not ranges: rows wrap).  The survivors'
// indices are appended to a list in LDS in their original order: a wave ballot, the wave
// counts through LDS, a prefix across the four waves, the rank of a lane among the set bits
// below it.  The order is the semantics.  A tile whose list stays empty returns without
// loading a flag; the others walk the LDS list only and read the record fields through a
// wave-uniform index, i.e. as scalar loads.  A sweep of 10^3 spheres therefore costs its own
// volume, not records x lattice.  The launch covers the local rows and the x range of the
// batch's bounding box only.
//
// Bit equality: the predicates are fp64 and perform the NumPy expressions operation for
// operation: (.5 + X) - x0, squares as t * t, sums as (a + b) + c, true divisions by the
// doubles the host divides by (R * R, max(n - 1, 1e-300) arrive as parameters), no fused
// multiply-adds (contraction is off for the whole file).
//
// The launcher returns 0 or a HIP error code and takes its stream explicitly.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int PAINT_BLOCK = 256, PAINT_WAVES = 4;
constexpr int TILE_X = 64, TILE_Y = PAINT_WAVES, TILE_Z = 4;
constexpr int PAINT_LIST = 4096;   // records per launch: the LDS list holds them all (uint16)

enum { K_BOX = 0, K_SPHERE, K_ELLIPSE, K_WEDGE, K_MASK, K_KINDS };
enum { MODE_OVERWRITE = 0, MODE_FILL, MODE_CHANGE };
// SPHERE opt: axes that enter the sum, the half-sphere y mapping, negation
enum { SPH_X = 1, SPH_Y = 2, SPH_Z = 4, SPH_HALF = 8, SPH_NOT = 16 };
// ELLIPSE opt: axis of term t (0 x, 1 y, 2 z, 3 none) in bits 2t, 2t + 1; the inner ellipse
constexpr int ELL_INNER = 64;

// the layout of ops.device.PAINT_REC
struct PaintRec {
  int32_t kind, mode;
  int32_t x0, x1, y0, y1, z0, z1;   // global box, half open, clipped to the lattice
  uint32_t fg, mask;
  int32_t opt;
  int32_t bit, outside;             // MASK: selected where byte & bit, `outside` off the window
  int32_t wx0, wy0, wz0, wnx, wny, wnz;
  int32_t pad;
  const unsigned char* ptr;         // MASK: (wnz, wny, wnx) bytes, strides sz, sy, 1
  long long sy, sz;
  double p[10];
};
static_assert(sizeof(PaintRec) == 184, "PaintRec is ops.device.PAINT_REC");

__device__ __forceinline__ double sq(double t) { return t * t; }

// _in_sphere of the normalised coordinates ((.5 + C) - d) / n; p: dx dy dz nx ny nz
__device__ __forceinline__ bool in_sphere(const PaintRec* r, double X, double Y, double Z) {
  const int o = r->opt;
  double xx = 0, yy = 0, zz = 0;
  if (o & SPH_X) xx = sq(2 * (((.5 + X) - r->p[0]) / r->p[3]) - 1);
  if (o & SPH_HALF)
    yy = sq(2 * (0.5 - (((.5 + Y) - r->p[1]) / r->p[4]) / 2.) - 1);
  else if (o & SPH_Y)
    yy = sq(2 * (((.5 + Y) - r->p[1]) / r->p[4]) - 1);
  if (o & SPH_Z) zz = sq(2 * (((.5 + Z) - r->p[2]) / r->p[5]) - 1);
  const bool in = (xx + yy) + zz < 1;
  return (o & SPH_NOT) ? !in : in;
}

// sum of ((.5 + C_t) - c_t)^2 / R2_t < lim [and the same numerators over R2i_t > 1];
// p: c[3] R2[3] lim R2i[3]
__device__ __forceinline__ bool in_ellipse(const PaintRec* r, double X, double Y, double Z) {
  const int o = r->opt;
  double s = 0, si = 0;
  for (int t = 0; t < 3; ++t) {
    const int a = (o >> (2 * t)) & 3;
    if (a == 3) break;
    const double C = a == 0 ? X : (a == 1 ? Y : Z);
    const double q = sq((.5 + C) - r->p[t]);
    const double e = q / r->p[3 + t];
    s = t == 0 ? e : s + e;
    if (o & ELL_INNER) {
      const double ei = q / r->p[7 + t];
      si = t == 0 ? ei : si + ei;
    }
  }
  return s < r->p[6] && (!(o & ELL_INNER) || si > 1.);
}

// _in_wedge; p: dx dy dz max(nx - 1, 1e-300) ...; opt: the direction, 8 = unknown (delta 0)
__device__ __forceinline__ bool in_wedge(const PaintRec* r, double X, double Y, double Z) {
  const double x = (X - r->p[0]) / r->p[3], y = (Y - r->p[1]) / r->p[4], z = (Z - r->p[2]) / r->p[5];
  double d;
  switch (r->opt) {
    case 0: d = x - y; break;
    case 1: d = (1. - x) - y; break;
    case 2: d = x - (1. - y); break;
    case 3: d = (1. - x) - (1. - y); break;
    case 4: d = x - z; break;
    case 5: d = (1. - x) - z; break;
    case 6: d = x - (1. - z); break;
    case 7: d = (1. - x) - (1. - z); break;
    default: d = 0; break;
  }
  return d < 1e-10;
}

__device__ __forceinline__ bool in_mask(const PaintRec* r, int x, int gy, int gz) {
  const int X = x - r->wx0, Y = gy - r->wy0, Z = gz - r->wz0;
  if (X < 0 || X >= r->wnx || Y < 0 || Y >= r->wny || Z < 0 || Z >= r->wnz) return r->outside != 0;
  return (r->ptr[Z * r->sz + Y * r->sy + X] & r->bit) != 0;
}

__global__ void __launch_bounds__(PAINT_BLOCK) k_paint(uint32_t* __restrict__ flags, int NY, int gnx,
                                                       const int* __restrict__ ys, const int* __restrict__ zs,
                                                       const PaintRec* __restrict__ recs, int n, int xa, int xb,
                                                       int ja, int jb, int ka, int kb) {
  __shared__ uint16_t list[PAINT_LIST];
  __shared__ int wcnt[PAINT_WAVES];
  __shared__ int tys[TILE_Y], tzs[TILE_Z];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tx0 = xa + blockIdx.x * TILE_X, tx1 = min(tx0 + TILE_X, xb);
  const int j0 = ja + blockIdx.y * TILE_Y, k0 = ka + blockIdx.z * TILE_Z;
  const int nj = min(TILE_Y, jb - j0), nk = min(TILE_Z, kb - k0);
  if (tid < nj) tys[tid] = ys[j0 + tid];
  if (tid >= 64 && tid - 64 < nk) tzs[tid - 64] = zs[k0 + tid - 64];
  __syncthreads();

  // cull: ordered compaction of the records that touch the tile
  int count = 0;
  for (int base = 0; base < n; base += PAINT_BLOCK) {
    const int i = base + tid;
    bool hit = false;
    if (i < n) {
      const PaintRec* r = recs + i;
      if (r->x0 < tx1 && r->x1 > tx0) {
        const int y0 = r->y0, y1 = r->y1, z0 = r->z0, z1 = r->z1;
        bool hy = false, hz = false;
        for (int a = 0; a < nj; ++a) hy |= tys[a] >= y0 && tys[a] < y1;
        for (int c = 0; c < nk; ++c) hz |= tzs[c] >= z0 && tzs[c] < z1;
        hit = hy && hz;
      }
    }
    const unsigned long long b = __ballot(hit);
    if (lane == 0) wcnt[wave] = __popcll(b);
    __syncthreads();
    int before = count;
    for (int w = 0; w < PAINT_WAVES; ++w) {
      const int c = wcnt[w];
      if (w < wave) before += c;
      count += c;
    }
    if (hit) list[before + __popcll(b & ((1ull << lane) - 1))] = (uint16_t)i;
    __syncthreads();
  }
  if (count == 0 || wave >= nj) return;

  // paint: wave `wave` owns row j0 + wave and marches the tile's planes
  const int x = tx0 + lane;
  const bool live = x < tx1;
  const int gy = __builtin_amdgcn_readfirstlane(tys[wave]);
  const double X = x, Y = gy;
  for (int c = 0; c < nk; ++c) {
    const int gz = __builtin_amdgcn_readfirstlane(tzs[c]);
    const double Z = gz;
    uint32_t* cell = flags + ((long long)(k0 + c) * NY + (j0 + wave)) * gnx + x;
    const uint32_t v0 = live ? *cell : 0;
    uint32_t v = v0;
    for (int q = 0; q < count; ++q) {
      const PaintRec* r = recs + __builtin_amdgcn_readfirstlane((int)list[q]);
      if (gy < r->y0 || gy >= r->y1 || gz < r->z0 || gz >= r->z1) continue;
      // x < x1 <= xb and x < tx0 + TILE_X: lanes past tx1 never pass
      bool sel = x >= r->x0 && x < r->x1;
      if (sel) {
        switch (r->kind) {
          case K_SPHERE: sel = in_sphere(r, X, Y, Z); break;
          case K_ELLIPSE: sel = in_ellipse(r, X, Y, Z); break;
          case K_WEDGE: sel = in_wedge(r, X, Y, Z); break;
          case K_MASK: sel = in_mask(r, x, gy, gz); break;
          default: break;
        }
      }
      const uint32_t m = r->mask;
      if (r->mode == MODE_FILL) sel = sel && (v & m) == 0;
      if (r->mode == MODE_CHANGE) sel = sel && (v & m) != 0;
      if (sel) v = (v & ~m) | r->fg;
    }
    if (live && v != v0) *cell = v;
  }
}

}  // namespace

// flags ((NZ, NY, gnx) uint32) painted with the n <= 4096 records recs (device, rec_bytes each)
// over the local rows [ja, jb) x planes [ka, kb) and x in [xa, xb), which hold every node of
// every record's box; ys[NY] / zs[NZ]: global coordinate of each local row / plane
extern "C" int tclb_paint(void* flags, int NZ, int NY, int gnx, const void* ys, const void* zs, const void* recs,
                          int n, int rec_bytes, int xa, int xb, int ja, int jb, int ka, int kb, void* stream) {
  if (n < 0 || n > PAINT_LIST || rec_bytes != (int)sizeof(PaintRec) || NZ < 0 || NY < 0 || gnx < 0)
    return (int)hipErrorInvalidValue;
  if (xa < 0 || xb > gnx || ja < 0 || jb > NY || ka < 0 || kb > NZ) return (int)hipErrorInvalidValue;
  if (n == 0 || xb <= xa || jb <= ja || kb <= ka) return 0;
  if (!flags || !ys || !zs || !recs) return (int)hipErrorInvalidDevicePointer;
  const dim3 grid((unsigned)((xb - xa + TILE_X - 1) / TILE_X), (unsigned)((jb - ja + TILE_Y - 1) / TILE_Y),
                  (unsigned)((kb - ka + TILE_Z - 1) / TILE_Z));
  if (grid.y > 65535u || grid.z > 65535u) return (int)hipErrorInvalidValue;
  k_paint<<<grid, dim3(PAINT_BLOCK), 0, (hipStream_t)stream>>>((uint32_t*)flags, NY, gnx, (const int*)ys,
                                                               (const int*)zs, (const PaintRec*)recs, n, xa, xb,
                                                               ja, jb, ka, kb);
  return (int)hipGetLastError();
}
