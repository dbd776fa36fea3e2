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
// Colour frames (tclb_amd/io/render.py write_png, device path): the (l, w) colour pair of a
// slice becomes a complete PNG file on the device, see "PNG frames" below.
//
// Every launcher returns 0 or a HIP error code and takes its stream explicitly.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

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

// ---- PNG frames ----------------------------------------------------------------------
//
// The (2, ny, nx) colour pair of a slice (Lattice.color) -> one RGBA8 PNG file in device
// memory: signature | IHDR | one IDAT | IEND.  The pixels are those of render.colormap,
// bit for bit; the file bytes are this coder's own (filter type 1, fixed Huffman codes).
//
//   k_frame_rows  one wave per scanline (image row r = lattice row ny-1-r), a lane per pixel,
//                 64 pixels a trip: colour map in fp32 without contraction, Sub filter from
//                 the left neighbour's lane (the chunk's last pixel is carried), deflate
//                 tokens at pixel granularity — a filtered pixel equal to its predecessor
//                 extends a run (ballot), the last lane of a run emits one length/distance
//                 match (distance 4, up to 256 bytes, overlapping copy), every other pixel
//                 four literals.  A wave prefix sum of the token lengths gives the bit
//                 offsets, the bits are ORed into an LDS staging buffer whose whole dwords
//                 go out with vector stores, the ragged rest is carried.  A row is one
//                 non-final fixed-Huffman block and an empty stored block, so it ends on a
//                 byte and rows compress independently into slots of the worst-case size
//                 (9 bits a byte).  The row also gives its Adler-32 partial.
//   hipcub        exclusive scan of the row lengths
//   k_png_pack    one wave per row: the slot to its place in the file (dword stores at the
//                 destination's alignment, the source funnel-shifted), and the row's CRC-32
//                 remainder: a lane multiplies its dword by x^(32 (64 - lane)) mod P, the
//                 wave XORs the products, the running remainder enters the next trip's
//                 first dword; the row's remainder is then moved to the end of the rows by
//                 the x^(8 n) mod P multiplication of zlib's crc32_combine
//   k_png_finish  Adler-32 partials joined in row order (a = a1 + a2 - 1, b = b1 + b2 +
//                 n2 (a1 - 1), mod 65521), row remainders XORed, header, trailer and the
//                 file's byte count written
//
// This is a run-length coder on purpose: no hash table, no dynamic codes, no match search
// beyond the previous pixel.

namespace {

constexpr int PNG_HEAD = 43;    // signature 8, IHDR chunk 25, IDAT length and type 8, zlib header 2
constexpr int PNG_TAIL = 22;    // final empty block 2, Adler-32 4, IDAT CRC 4, IEND chunk 12
constexpr int PNG_STAGE = 80;   // dwords of a wave's staging buffer: 31 carried bits + 64 tokens of <= 47
constexpr uint32_t CRC_POLY = 0xedb88320u;
constexpr uint32_t ADLER_MOD = 65521u;

// a * b mod P of the reflected CRC-32 polynomials (bit 31 is x^0)
__host__ __device__ inline uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; i++) {
    p ^= b & (0u - ((a >> (31 - i)) & 1u));
    b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
  }
  return p;
}

// x^e mod P
__host__ __device__ inline uint32_t crc_xpow(unsigned long long e) {
  uint32_t p = 0x80000000u, b = 0x40000000u;
  for (; e; e >>= 1) {
    if (e & 1u) p = crc_mul(p, b);
    b = crc_mul(b, b);
  }
  return p;
}

// running CRC state c after one more byte
__host__ __device__ inline uint32_t crc_byte(uint32_t c, uint32_t v) {
  c ^= v;
  for (int i = 0; i < 8; i++) c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1u)));
  return c;
}

// Adler-32 (a1, b1) of n1 bytes followed by (a2, b2) of n2 bytes, each started at (1, 0)
__host__ __device__ inline void adler_join(uint32_t& a1, uint32_t& b1, unsigned long long& n1, uint32_t a2,
                                           uint32_t b2, unsigned long long n2) {
  const uint32_t am = (a1 + ADLER_MOD - 1u) % ADLER_MOD;
  b1 = (uint32_t)(((unsigned long long)b1 + b2 + (n2 % ADLER_MOD) * am) % ADLER_MOD);
  a1 = (am + a2) % ADLER_MOD;
  n1 += n2;
}

// most bytes of a compressed row: block header 3 bits, filter byte 8, 36 a pixel, end of
// block 7, stored header 3, padding to a byte, LEN / NLEN 4 bytes
__host__ __device__ inline long long png_row_max(int nx) { return (36LL * nx + 21 + 7) / 8 + 4; }
// a row's slot: the last flush writes whole dwords and the pack reads one dword ahead
__host__ __device__ inline long long png_slot(int nx) { return (png_row_max(nx) + 8 + 15) / 16 * 16; }

// render.colormap operation for operation as the tensor ops evaluate it on the device:
// every product and sum rounded on its own, a division by a constant as the product with
// its fp32 reciprocal
__device__ __forceinline__ uint32_t png_colour(float l, float w) {
#pragma clang fp contract(off)
  const float r100 = 1.0f / 100.0f, r10 = 1.0f / 10.0f;
  const float s = l * 111.0f;
  float r = 0.0f, g = 0.0f, b = 0.0f;
  if (s < -111.0f) r = g = b = 255.0f;
  if (s >= -111.0f && s < -11.0f) r = truncf(255.0f * (-s - 11.0f) * r100), g = 255.0f, b = 255.0f;
  if (s >= -11.0f && s < -1.0f) r = 0.0f, g = truncf(255.0f * (-s - 1.0f) * r10), b = 255.0f;
  if (s >= -1.0f && s < 0.0f) r = 0.0f, g = 0.0f, b = truncf(255.0f * (-s));
  if (s >= 0.0f && s < 1.0f) r = truncf(255.0f * s), g = 0.0f, b = 0.0f;
  if (s >= 1.0f && s < 11.0f) r = 255.0f, g = truncf(255.0f * (s - 1.0f) * r10), b = 0.0f;
  if (s >= 11.0f && s < 111.0f) r = 255.0f, g = 255.0f, b = truncf(255.0f * (s - 11.0f) * r100);
  if (s >= 111.0f) r = g = b = 255.0f;
  r = truncf(r * w);
  const float gw = g * w, bg = (1.0f - w) * 255.0f;
  g = truncf(gw + bg);
  b = truncf(b * w);
  if (!isfinite(s)) r = 255.0f, g = 0.0f, b = 255.0f;
  r = fminf(fmaxf(r, 0.0f), 255.0f);
  g = fminf(fmaxf(g, 0.0f), 255.0f);
  b = fminf(fmaxf(b, 0.0f), 255.0f);
  return (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16) | 0xff000000u;
}

// p - q on each of the four bytes, mod 256
__device__ __forceinline__ uint32_t sub_bytes(uint32_t p, uint32_t q) {
  const uint32_t h = 0x80808080u;
  return ((p | h) - (q & ~h)) ^ ((p ^ ~q) & h);
}

// fixed Huffman code of literal v appended at bit n of acc (codes go in most significant bit first)
__device__ __forceinline__ void put_literal(unsigned long long& acc, int& n, uint32_t v) {
  const uint32_t code = v < 144u ? 0x30u + v : 0x190u + (v - 144u);
  const int len = v < 144u ? 8 : 9;
  acc |= (unsigned long long)(__brev(code) >> (32 - len)) << n;
  n += len;
}

// match of k pixels (4 k bytes, k = 1 .. 64) at distance 4: length code, its extra bits,
// distance code 3 (five bits, no extra)
__device__ __forceinline__ void put_match(unsigned long long& acc, int& n, int k) {
  const uint32_t v = 4u * (uint32_t)k - 3u;
  uint32_t sym = 257u + v, e = 0u;
  if (v >= 8u) {
    e = 29u - (uint32_t)__clz(v);                       // floor(log2 v) - 2 extra bits
    sym = 257u + 4u * (e + 1u) + ((v - (4u << e)) >> e);
  }
  const uint32_t code = sym < 280u ? sym - 256u : 0xc0u + (sym - 280u);
  const int len = sym < 280u ? 7 : 8;
  const uint32_t bits = (__brev(code) >> (32 - len)) | ((v & ((1u << e) - 1u)) << len) | (24u << (len + e));
  acc |= (unsigned long long)bits << n;
  n += len + (int)e + 5;
}

// nb bits of acc ORed into the staging buffer at bit `pos`
__device__ __forceinline__ void stage_or(uint32_t* stage, int pos, unsigned long long acc) {
  const int wi = pos >> 5, sh = pos & 31;
  const uint32_t w0 = (uint32_t)acc << sh, w1 = (uint32_t)(acc >> (32 - sh));
  const uint32_t w2 = sh ? (uint32_t)(acc >> (64 - sh)) : 0u;
  if (w0) atomicOr(&stage[wi], w0);
  if (w1) atomicOr(&stage[wi + 1], w1);
  if (w2) atomicOr(&stage[wi + 2], w2);
}

// lw: l plane then w plane, (ny, nx) each.  slots: ny slots of `slot` bytes; len[r]: bytes of
// row r's deflate data, len[ny] = 0 for the scan; adl[r]: Adler-32 (a, b) of row r's 4 nx + 1
// filtered bytes; pix (may be null): the image's pixels, (ny, nx) RGBA dwords
template <class T>
__global__ void __launch_bounds__(64) k_frame_rows(const T* __restrict__ lw, int nx, int ny,
                                                   unsigned char* __restrict__ slots, long long slot,
                                                   long long* __restrict__ len, uint2* __restrict__ adl,
                                                   uint32_t* __restrict__ pix) {
  __shared__ uint32_t stage[PNG_STAGE];
  const int r = (int)blockIdx.x, lane = (int)threadIdx.x;
  const T* L = lw + (long long)(ny - 1 - r) * nx;
  const T* W = L + (long long)nx * ny;
  uint32_t* dst = (uint32_t*)(slots + (long long)r * slot);
  for (int i = lane; i < PNG_STAGE; i += 64) stage[i] = 0u;
  __syncthreads();
  long long words = 0;                 // dwords of the row already in its slot
  int carry = 0;                       // bits waiting in stage[0]
  uint32_t last_p = 0u, last_f = 0u;   // the previous chunk's last pixel, raw and filtered
  unsigned long long sa = 0ull, sb = 0ull;
  for (int x0 = 0; x0 < nx; x0 += 64) {
    const int x = x0 + lane;
    const bool valid = x < nx;
    const uint32_t p = valid ? png_colour((float)L[x], (float)W[x]) : 0u;
    if (pix && valid) pix[(long long)r * nx + x] = p;
    uint32_t left = __shfl_up(p, 1);
    if (lane == 0) left = last_p;
    const uint32_t f = sub_bytes(p, left);
    uint32_t fl = __shfl_up(f, 1);
    if (lane == 0) fl = last_f;
    const bool eq = valid && x > 0 && f == fl;
    const unsigned long long E = __ballot(eq);
    const bool run_end = eq && (lane == 63 || !((E >> (lane + 1)) & 1ull));
    unsigned long long acc = 0ull;
    int nb = 0;
    if (valid && !eq) {
      if (x == 0) {                    // block header (not final, fixed codes) and the filter byte
        acc = 2ull, nb = 3;
        put_literal(acc, nb, 1u);
      }
      put_literal(acc, nb, f & 0xffu);
      put_literal(acc, nb, (f >> 8) & 0xffu);
      put_literal(acc, nb, (f >> 16) & 0xffu);
      put_literal(acc, nb, f >> 24);
    } else if (run_end) {
      const unsigned long long ones = ~(E << (63 - lane));     // the run's bits end at bit 63
      put_match(acc, nb, ones ? __clzll((long long)ones) : 64);
    }
    if (valid) {                       // bytes at 1 + 4 x + c of the n = 4 nx + 1 of the row, weight n - position
      const unsigned long long d0 = f & 0xffu, d1 = (f >> 8) & 0xffu, d2 = (f >> 16) & 0xffu, d3 = f >> 24;
      sa += d0 + d1 + d2 + d3;
      sb += 4ull * (unsigned long long)(nx - x) * (d0 + d1 + d2 + d3) - (d1 + 2ull * d2 + 3ull * d3);
      if (sb >> 62) sb %= ADLER_MOD;
    }
    int inc = nb;
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(inc, d);
      if (lane >= d) inc += t;
    }
    const int tot = carry + __shfl(inc, 63);
    if (nb) stage_or(stage, carry + inc - nb, acc);
    __syncthreads();
    const int nfull = tot >> 5;        // <= 73
    for (int i = lane; i < nfull; i += 64) dst[words + i] = stage[i];
    const uint32_t rest = stage[nfull];
    __syncthreads();
    for (int i = lane; i < PNG_STAGE; i += 64) stage[i] = i == 0 ? rest : 0u;
    __syncthreads();
    words += nfull;
    carry = tot & 31;
    last_p = __shfl(p, 63);
    last_f = __shfl(f, 63);
  }
  // end of block (7 zero bits), empty stored block: header 3 zero bits, padding to a byte,
  // LEN 0, NLEN 0xffff
  const int pad = (carry + 10 + 7) & ~7;
  if (lane == 0) stage_or(stage, pad, 0xffff0000ull);
  __syncthreads();
  const int nlast = (pad + 32 + 31) >> 5;
  if (lane < nlast) dst[words + lane] = stage[lane];
  sa %= ADLER_MOD;
  sb %= ADLER_MOD;
  uint32_t a = (uint32_t)sa, b = (uint32_t)sb;
  for (int d = 32; d; d >>= 1) a += __shfl_xor(a, d), b += __shfl_xor(b, d);
  if (lane == 0) {
    const unsigned long long n = 4ull * (unsigned long long)nx + 1ull;   // the filter byte is 1, at weight n
    len[r] = words * 4 + (pad + 32) / 8;
    adl[r] = make_uint2((uint32_t)((a + 2ull) % ADLER_MOD), (uint32_t)((b + 2ull * n) % ADLER_MOD));
    if (r == 0) len[ny] = 0;
  }
}

// row r's len[r] bytes from its slot to out + PNG_HEAD + off[r]; part[r]: the row's CRC-32
// remainder times x^(8 * bytes of the rows behind it)
__global__ void __launch_bounds__(64) k_png_pack(const unsigned char* __restrict__ slots, long long slot,
                                                 const long long* __restrict__ len,
                                                 const long long* __restrict__ off, int ny,
                                                 unsigned char* __restrict__ out, uint32_t* __restrict__ part) {
  const int r = (int)blockIdx.x, lane = (int)threadIdx.x;
  const unsigned char* src = slots + (long long)r * slot;
  const uint32_t* W = (const uint32_t*)src;
  const long long n = len[r];
  unsigned char* d = out + PNG_HEAD + off[r];
  long long head = (long long)((4u - (unsigned)((uintptr_t)d & 3u)) & 3u);
  if (head > n) head = n;
  if (lane < head) d[lane] = src[lane];
  const long long nw = (n - head) >> 2;
  uint32_t* dw = (uint32_t*)(d + head);
  for (long long k = lane; k < nw; k += 64) dw[k] = __builtin_amdgcn_alignbyte(W[k + 1], W[k], (uint32_t)head);
  const long long done = head + 4 * nw;
  if (lane < n - done) d[done + lane] = src[done + lane];
  // remainder of the q whole dwords, zero dwords in front up to a multiple of 64 (they do
  // not change a remainder), then the last bytes one by one
  const long long q = n >> 2;
  const long long front = (64 - (q & 63)) & 63;
  const uint32_t mult = crc_xpow(32ull * (unsigned long long)(64 - lane));
  uint32_t c = 0u;
  for (long long base = -front; base < q; base += 64) {
    const long long j = base + lane;
    uint32_t v = j >= 0 ? W[j] : 0u;
    if (lane == 0) v ^= c;
    v = crc_mul(v, mult);
    for (int s = 32; s; s >>= 1) v ^= __shfl_xor(v, s);
    c = v;
  }
  for (long long k = 4 * q; k < n; k++) c = crc_byte(c, src[k]);
  if (lane == 0) part[r] = crc_mul(c, crc_xpow(8ull * (unsigned long long)(off[ny] - off[r] - n)));
}

__device__ inline unsigned char* put_be32(unsigned char* p, uint32_t v) {
  p[0] = (unsigned char)(v >> 24), p[1] = (unsigned char)(v >> 16), p[2] = (unsigned char)(v >> 8);
  p[3] = (unsigned char)v;
  return p + 4;
}

// everything of the file around the rows; *nbytes: the file's bytes, or -1 where the IDAT
// chunk would pass the format's 2^31 - 1
__global__ void __launch_bounds__(256) k_png_finish(int nx, int ny, const long long* __restrict__ off,
                                                    const uint2* __restrict__ adl,
                                                    const uint32_t* __restrict__ part,
                                                    unsigned char* __restrict__ out, long long* nbytes) {
  __shared__ uint32_t sa[256], sb[256], sx[256];
  __shared__ unsigned long long sn[256];
  const int t = (int)threadIdx.x;
  const long long per = ((long long)ny + 255) / 256;
  const unsigned long long rown = 4ull * (unsigned long long)nx + 1ull;
  uint32_t a = 1u, b = 0u, x = 0u;
  unsigned long long n = 0ull;
  for (long long r = t * per; r < (t + 1) * per && r < ny; r++) {
    adler_join(a, b, n, adl[r].x, adl[r].y, rown);
    x ^= part[r];
  }
  sa[t] = a, sb[t] = b, sn[t] = n, sx[t] = x;
  __syncthreads();
  for (int s = 1; s < 256; s <<= 1) {
    if ((t & (2 * s - 1)) == 0) {
      adler_join(sa[t], sb[t], sn[t], sa[t + s], sb[t + s], sn[t + s]);
      sx[t] ^= sx[t + s];
    }
    __syncthreads();
  }
  if (t != 0) return;
  const long long S = off[ny];
  if (S + 8 > 0x7fffffffLL) {                           // zlib header 2, rows, final block 2, Adler-32 4
    *nbytes = -1;
    return;
  }
  static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  unsigned char* p = out;
  for (int i = 0; i < 8; i++) *p++ = sig[i];
  p = put_be32(p, 13u);
  unsigned char* ihdr = p;
  *p++ = 'I', *p++ = 'H', *p++ = 'D', *p++ = 'R';
  p = put_be32(p, (uint32_t)nx);
  p = put_be32(p, (uint32_t)ny);
  *p++ = 8, *p++ = 6, *p++ = 0, *p++ = 0, *p++ = 0;     // 8 bits, RGBA, deflate, filter method 0, no interlace
  uint32_t c = 0xffffffffu;
  for (int i = 0; i < 17; i++) c = crc_byte(c, ihdr[i]);
  p = put_be32(p, ~c);
  p = put_be32(p, (uint32_t)(S + 8));
  unsigned char* idat = p;
  *p++ = 'I', *p++ = 'D', *p++ = 'A', *p++ = 'T', *p++ = 0x78, *p++ = 0x01;
  c = 0xffffffffu;
  for (int i = 0; i < 6; i++) c = crc_byte(c, idat[i]);
  c = crc_mul(c, crc_xpow(8ull * (unsigned long long)S)) ^ sx[0];
  p += S;
  unsigned char* tail = p;
  *p++ = 0x03, *p++ = 0x00;                             // final block, fixed codes, end of block
  p = put_be32(p, (sb[0] << 16) | sa[0]);
  for (int i = 0; i < 6; i++) c = crc_byte(c, tail[i]);
  p = put_be32(p, ~c);
  p = put_be32(p, 0u);
  *p++ = 'I', *p++ = 'E', *p++ = 'N', *p++ = 'D';
  p = put_be32(p, 0xae426082u);
  *nbytes = (long long)(p - out);
}

size_t png_align(size_t b) { return (b + 255) / 256 * 256; }

size_t png_scan_bytes(int ny) {
  size_t b = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (long long*)nullptr, (long long*)nullptr, ny + 1);
  return b;
}

bool png_sizes_ok(int nx, int ny) { return nx > 0 && ny > 0 && (long long)nx * ny * 4 + ny < 0x80000000LL; }

}  // namespace

// bytes of the largest file (*out_bytes) and of the scratch buffer (*scratch_bytes) of an
// nx x ny frame
extern "C" int tclb_enc_png_bytes(int nx, int ny, long long* out_bytes, long long* scratch_bytes) {
  if (!png_sizes_ok(nx, ny) || !out_bytes || !scratch_bytes) return (int)hipErrorInvalidValue;
  *out_bytes = PNG_HEAD + PNG_TAIL + (long long)ny * png_row_max(nx);
  *scratch_bytes = (long long)(png_align((size_t)ny * (size_t)png_slot(nx)) + 2 * png_align(8 * ((size_t)ny + 1)) +
                               png_align(8 * (size_t)ny) + png_align(4 * (size_t)ny) + png_align(png_scan_bytes(ny)));
  return 0;
}

// PNG file of the colour pair lw ((2, ny, nx), elements of elem = 4 or 8 bytes: fp32 or fp64)
// at `out`; scratch: 256-byte aligned; both of at least the bytes tclb_enc_png_bytes gives.
// pixels (may be null): the image as (ny, nx) RGBA.  *nbytes (device or pinned word): the
// file's bytes once the stream has run, -1 where the frame does not fit one IDAT chunk.
extern "C" int tclb_enc_png(const void* lw, int elem, int nx, int ny, void* out, long long out_bytes, void* scratch,
                            long long scratch_bytes, void* pixels, long long* nbytes, void* stream) {
  long long need_out = 0, need_scratch = 0;
  if (tclb_enc_png_bytes(nx, ny, &need_out, &need_scratch) != 0 || (elem != 4 && elem != 8))
    return (int)hipErrorInvalidValue;
  if (out_bytes < need_out || scratch_bytes < need_scratch) return (int)hipErrorInvalidValue;
  if (!lw || !out || !scratch || !nbytes || ((uintptr_t)lw & (uintptr_t)(elem - 1)) || ((uintptr_t)scratch & 255u) ||
      ((uintptr_t)pixels & 3u) || ((uintptr_t)nbytes & 7u))
    return (int)hipErrorInvalidDevicePointer;
  hipStream_t s = (hipStream_t)stream;
  const long long slot = png_slot(nx);
  char* p = (char*)scratch;
  unsigned char* slots = (unsigned char*)p;
  p += png_align((size_t)ny * (size_t)slot);
  long long* len = (long long*)p;
  p += png_align(8 * ((size_t)ny + 1));
  long long* off = (long long*)p;
  p += png_align(8 * ((size_t)ny + 1));
  uint2* adl = (uint2*)p;
  p += png_align(8 * (size_t)ny);
  uint32_t* part = (uint32_t*)p;
  p += png_align(4 * (size_t)ny);
  size_t tb = png_scan_bytes(ny);
  if (elem == 4)
    k_frame_rows<float><<<dim3((unsigned)ny), dim3(64), 0, s>>>((const float*)lw, nx, ny, slots, slot, len, adl,
                                                               (uint32_t*)pixels);
  else
    k_frame_rows<double><<<dim3((unsigned)ny), dim3(64), 0, s>>>((const double*)lw, nx, ny, slots, slot, len, adl,
                                                                (uint32_t*)pixels);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  if ((e = hipcub::DeviceScan::ExclusiveSum(p, tb, len, off, ny + 1, s)) != hipSuccess) return (int)e;
  k_png_pack<<<dim3((unsigned)ny), dim3(64), 0, s>>>(slots, slot, len, off, ny, (unsigned char*)out, part);
  k_png_finish<<<dim3(1), dim3(256), 0, s>>>(nx, ny, off, adl, part, (unsigned char*)out, nbytes);
  return (int)hipGetLastError();
}
