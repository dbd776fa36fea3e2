// Device-side encoding of VTK payloads (tclb_amd/io/vtk.py write_vti_device): the gathered
// output fields already lie on the device in the layout and element type of the file, so
// the byte shuffling that turns them into the file's text runs here at memory speed and
// the host only writes finished ASCII.
//
//   k_b64          base64 (RFC 4648, standard alphabet, '=' padding) of a byte range
//   k_flag_groups  every flag-group array ((flag & mask) >> shift as uint8) of a window of
//                  the strided flag array in one pass
//
// k_b64, work split: one lane owns one 12-byte group — one dwordx3 load, 16 characters, one
// dwordx4 store — so a wave reads 768 contiguous bytes and writes 1 024 contiguous bytes per
// item.  A thread takes B64_ITEMS items per loop trip, a block's trip covers
// B64_BLOCK * B64_ITEMS consecutive groups (item u of lane t is group u * B64_BLOCK + t of
// the trip: every load and store of a wave is one contiguous run), and the grid strides
// over the trips.  All loads of a trip are issued before the first character is formed.
// The text is written once and read by the copy engine: non-temporal stores.
//
// k_b64, encoding in registers: four byte permutes (v_perm_b32) pick the big-endian 24-bit
// groups out of the three little-endian dwords; shifts and masks spread each group into
// four sextets, one per byte of a dword, in text order.  Sextet -> ASCII is arithmetic on
// all four bytes of the dword at once: the sextets are below 64, so adding (128 - k) to
// every byte sets bit 7 exactly in the bytes >= k with no carry between bytes, and the
// piecewise offsets (+65, +71 from 26, -4 from 52, -19 at 62, -16 at 63) are the base 65
// plus the steps +6, -75, -15, +3 times those compare bits.  The steps are applied in an
// order in which no byte leaves 0..255, so whole-dword adds and subtracts never carry or
// borrow across bytes.  This is the form kept: it needs no table, neither in global memory
// nor in LDS.  An LDS-table variant was not built: with this form the device side of a
// whole-lattice write already hides under the file write (profiles/README.md, r08a).
//
// Every launcher returns 0 or a HIP error code and takes its stream explicitly.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int B64_BLOCK = 256;
constexpr int B64_ITEMS = 4;

// 12 input bytes / 16 output characters at the 4-byte alignment the launcher checks
struct __attribute__((aligned(4))) In12 { uint32_t w[3]; };
typedef uint32_t Out16 __attribute__((ext_vector_type(4), aligned(4)));

// four sextets (one per byte, each < 64) -> their four base64 characters
__device__ __forceinline__ uint32_t b64_chars(uint32_t v) {
  const uint32_t ones = 0x01010101u;
  const uint32_t ge26 = ((v + (128 - 26) * ones) >> 7) & ones;
  const uint32_t ge52 = ((v + (128 - 52) * ones) >> 7) & ones;
  const uint32_t ge62 = ((v + (128 - 62) * ones) >> 7) & ones;
  const uint32_t ge63 = ((v + (128 - 63) * ones) >> 7) & ones;
  uint32_t c = v + 65 * ones + 6 * ge26;   // A-Z, a-z (+71)
  c -= 75 * ge52;                          // 0-9: +71 - 75 = -4 (v + 71 >= 123 there)
  c -= 15 * ge62;                          // '+': -19 (v - 4 >= 58 there)
  c += 3 * ge63;                           // '/': -16
  return c;
}

// a 24-bit big-endian group (bits 23..0) -> its four characters in text (memory) order
__device__ __forceinline__ uint32_t b64_group(uint32_t g) {
  const uint32_t v = (g >> 18) | ((g >> 4) & 0x3f00u) | ((g << 10) & 0x3f0000u) | ((g << 24) & 0x3f000000u);
  return b64_chars(v);
}

// v_perm_b32: selector bytes 0-3 pick the bytes of `lo`, 4-7 those of `hi`, 0x0c is zero
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) {
  return __builtin_amdgcn_perm(hi, lo, sel);
}

__device__ __forceinline__ Out16 b64_encode12(const In12& in) {
  const uint32_t w0 = in.w[0], w1 = in.w[1], w2 = in.w[2];   // bytes b0..b3, b4..b7, b8..b11
  Out16 o;
  o.x = b64_group(perm(0u, w0, 0x0c000102u));   // b0 b1 b2
  o.y = b64_group(perm(w1, w0, 0x0c030405u));   // b3 b4 b5
  o.z = b64_group(perm(w2, w1, 0x0c020304u));   // b6 b7 b8
  o.w = b64_group(perm(0u, w2, 0x0c010203u));   // b9 b10 b11
  return o;
}

__device__ __forceinline__ char b64_char1(uint32_t s) { return (char)(b64_chars(s) & 0xffu); }

// ngroups full 12-byte groups, then `tail` (0-11) more bytes encoded by one lane
__global__ void __launch_bounds__(B64_BLOCK) k_b64(const unsigned char* __restrict__ src,
                                                   unsigned char* __restrict__ dst, long long ngroups, int tail) {
  const In12* in = (const In12*)src;
  Out16* out = (Out16*)dst;
  const long long per_trip = (long long)B64_BLOCK * B64_ITEMS;
  for (long long base = (long long)blockIdx.x * per_trip; base < ngroups; base += (long long)gridDim.x * per_trip) {
    const long long g0 = base + threadIdx.x;
    In12 v[B64_ITEMS];
    if (base + per_trip <= ngroups) {
#pragma unroll
      for (int u = 0; u < B64_ITEMS; u++) v[u] = in[g0 + u * B64_BLOCK];
#pragma unroll
      for (int u = 0; u < B64_ITEMS; u++) __builtin_nontemporal_store(b64_encode12(v[u]), out + g0 + u * B64_BLOCK);
    } else {
#pragma unroll
      for (int u = 0; u < B64_ITEMS; u++)
        if (g0 + u * B64_BLOCK < ngroups) v[u] = in[g0 + u * B64_BLOCK];
#pragma unroll
      for (int u = 0; u < B64_ITEMS; u++)
        if (g0 + u * B64_BLOCK < ngroups)
          __builtin_nontemporal_store(b64_encode12(v[u]), out + g0 + u * B64_BLOCK);
    }
  }
  if (tail && blockIdx.x == 0 && threadIdx.x == 0) {
    const unsigned char* s = src + ngroups * 12;
    unsigned char* d = dst + ngroups * 16;
    for (int k = 0; k < tail; k += 3, d += 4) {
      const int m = tail - k < 3 ? tail - k : 3;          // bytes of this group: 1, 2 or 3
      uint32_t g = (uint32_t)s[k] << 16;
      if (m > 1) g |= (uint32_t)s[k + 1] << 8;
      if (m > 2) g |= (uint32_t)s[k + 2];
      d[0] = b64_char1(g >> 18);
      d[1] = b64_char1((g >> 12) & 63u);
      d[2] = m > 1 ? b64_char1((g >> 6) & 63u) : '=';
      d[3] = m > 2 ? b64_char1(g & 63u) : '=';
    }
  }
}

// ---- flag groups ---------------------------------------------------------------------

constexpr int FG_MAX = 16;

struct FlagGroups {
  uint32_t mask[FG_MAX];
  uint32_t shift[FG_MAX];
  unsigned char* out[FG_MAX];
};

// window (wx, wy, wz) of the flag array at `f` (row stride sy, plane stride sz, elements);
// lane d writes bytes 4d..4d+3 of every group's contiguous (wz, wy, wx) array: the flags of
// those four nodes are loaded once and reused for every group.  A window row need not be a
// multiple of four, so each of the four indices has its own (x, y, z).
template <class T>
__global__ void __launch_bounds__(256) k_flag_groups(const T* __restrict__ f, long long sy, long long sz, int wx,
                                                     int wy, long long total, int ng, FlagGroups G) {
  const long long d = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long i0 = d * 4;
  if (i0 >= total) return;
  uint32_t v[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const long long i = i0 + k;
    v[k] = 0;
    if (i < total) {
      long long z;
      int x, y;
      if (total <= 0x7fffffffLL) {          // 32-bit divisions where the window allows it
        const uint32_t row = (uint32_t)i / (uint32_t)wx, zz = row / (uint32_t)wy;
        x = (int)((uint32_t)i - row * (uint32_t)wx);
        y = (int)(row - zz * (uint32_t)wy);
        z = zz;
      } else {
        const long long row = i / wx;
        z = row / wy;
        x = (int)(i - row * wx);
        y = (int)(row - z * wy);
      }
      v[k] = (uint32_t)f[z * sz + y * sy + x];    // T is unsigned: no sign extension
    }
  }
  const bool whole = i0 + 4 <= total;
  for (int g = 0; g < ng; g++) {
    const uint32_t m = G.mask[g], s = G.shift[g];
    const uint32_t b0 = ((v[0] & m) >> s) & 0xffu, b1 = ((v[1] & m) >> s) & 0xffu;
    const uint32_t b2 = ((v[2] & m) >> s) & 0xffu, b3 = ((v[3] & m) >> s) & 0xffu;
    unsigned char* o = G.out[g] + i0;
    if (whole) {
      __builtin_nontemporal_store(b0 | (b1 << 8) | (b2 << 16) | (b3 << 24), (uint32_t*)o);
    } else {                                // the ragged last dword
      o[0] = (unsigned char)b0;
      if (i0 + 1 < total) o[1] = (unsigned char)b1;
      if (i0 + 2 < total) o[2] = (unsigned char)b2;
    }
  }
}

template <class T>
int flag_groups(const void* f, long long sy, long long sz, int wx, int wy, long long total, int ng,
                const FlagGroups& G, hipStream_t s) {
  const long long blocks = ((total + 3) / 4 + 255) / 256;
  if (blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  k_flag_groups<T><<<dim3((unsigned)blocks), dim3(256), 0, s>>>((const T*)f, sy, sz, wx, wy, total, ng, G);
  return (int)hipGetLastError();
}

}  // namespace

// base64 of n bytes at src (4-byte aligned) into 4 * ceil(n / 3) characters at dst (4-byte
// aligned); a misaligned pointer is an error
extern "C" int tclb_enc_b64(const void* src, void* dst, long long n, void* stream) {
  if (n < 0) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  if (!src || !dst || ((uintptr_t)src & 3u) || ((uintptr_t)dst & 3u)) return (int)hipErrorInvalidDevicePointer;
  const long long ngroups = n / 12;
  const int tail = (int)(n - ngroups * 12);
  const long long per_trip = (long long)B64_BLOCK * B64_ITEMS;
  long long blocks = (ngroups + per_trip - 1) / per_trip;
  if (blocks < 1) blocks = 1;
  // a few trips per block on large inputs: 256 CUs x 8 resident blocks
  if (blocks > 2048 * 4) blocks = 2048 * 4;
  k_b64<<<dim3((unsigned)blocks), dim3(B64_BLOCK), 0, (hipStream_t)stream>>>(
      (const unsigned char*)src, (unsigned char*)dst, ngroups, tail);
  return (int)hipGetLastError();
}

// ng (<= 16) flag-group arrays of the window (wx, wy, wz) at `flags` (elements of flag_bits
// 16 or 32, read as unsigned; strides in elements, x contiguous): out[g][i] =
// ((flag_i & mask[g]) >> shift[g]) as uint8, i over (z, y, x) of the window; every out[g]
// is 4-byte aligned
extern "C" int tclb_enc_flag_groups(const void* flags, int flag_bits, long long sy, long long sz, int wx, int wy,
                                    int wz, int ng, const unsigned* mask, const unsigned* shift, void* const* out,
                                    void* stream) {
  if (ng < 0 || ng > FG_MAX || wx < 0 || wy < 0 || wz < 0 || (flag_bits != 16 && flag_bits != 32))
    return (int)hipErrorInvalidValue;
  const long long total = (long long)wx * wy * wz;
  if (total == 0 || ng == 0) return 0;
  if (!flags || !mask || !shift || !out) return (int)hipErrorInvalidValue;
  FlagGroups G = {};
  for (int g = 0; g < ng; g++) {
    if (!out[g] || ((uintptr_t)out[g] & 3u)) return (int)hipErrorInvalidDevicePointer;
    if (shift[g] > 31u) return (int)hipErrorInvalidValue;
    G.mask[g] = mask[g];
    G.shift[g] = shift[g];
    G.out[g] = (unsigned char*)out[g];
  }
  if (flag_bits == 16) return flag_groups<uint16_t>(flags, sy, sz, wx, wy, total, ng, G, (hipStream_t)stream);
  return flag_groups<uint32_t>(flags, sy, sz, wx, wy, total, ng, G, (hipStream_t)stream);
}
