// Baseline JPEG encoding of a batch of packed RGB images, entirely on the device: what
// `PIL.Image.fromarray(rgb).save(path)` writes with libjpeg-turbo's defaults -- quality 75, 4:2:0, the Annex K Huffman tables, no
// restart markers -- byte for byte.  Every stage of that encoder is integer arithmetic, restated here from the IJG / libjpeg-turbo
// sources: jccolor.c rgb_ycc_convert, jcsample.c h2v2_downsample with its edge expansion, jfdctint.c jpeg_fdct_islow,
// jcdctmgr.c quantisation, jccoefct.c's dummy blocks, jchuff.c encode_one_block / flush_bits.  An encoder has no sequential pass:
// a block's bits depend on that block and one neighbouring DC value, and where they go is a prefix sum.
//
//   front end   one thread = one 8x8 block, in scan order (MCU after MCU, Y00 Y01 Y10 Y11 Cb Cr): colour conversion, edge
//               replication, chroma downsampling, forward DCT, quantisation -> int16 [64] in zigzag order
//   lengths     one thread = one block: the number of bits its Huffman codes take
//   scan        exclusive prefix sum of the lengths over all blocks of the batch (tiles of 1024, three launches)
//   layout      per image: bits, bytes, first word of its bit stream in the packed-word buffer (streams start on 32-bit words)
//   pack        one thread = one block: the codes again, shifted to their bit offset; whole words it fills are stored, the first
//               and the last, which it shares with its neighbours, are OR-ed atomically into the zeroed buffer; the last block
//               of an image appends the 1-bit pad
//   stuffing    FF bytes per tile of 1024 words, their prefix sum, per-image stuffed byte counts (the end of call 1); then, in
//               call 2, every byte moved to its final place with a 00 behind every FF, each thread owning the bytes it writes
// The caller reads the n byte counts between the calls and sizes the output exactly.  The packed-word buffer is sized for the
// worst block the tables admit (1658 bits), so no capacity is ever a guess.  Nothing is allocated, nothing synchronises.
#include "block_ops.h"

namespace {

constexpr int ENC_TILE = 1024;                    // elements per scan tile: 256 threads x 4
constexpr int ENC_BLOCK_WORDS = 52;               // 20 bits of DC + 63 x (16 + 10) bits of AC = 1658 bits <= 52 words
constexpr int ENC_CHUNK = 64;                     // images whose geometry travels in one launch's kernel arguments

constexpr int kZig[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K quantisation tables (natural order) and Huffman specifications: code counts per length, then the symbols
constexpr int kStdQ[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
constexpr unsigned char kDcCounts[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr unsigned char kAcCounts[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr unsigned char kAcSyms[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// what the kernels read: quantiser divisors q << 3 of quality 75 (jcparam.c jpeg_quality_scaling: scale 50), and per symbol
// code | length << 16 (jchuff.c jpeg_make_c_derived_tbl); [0] luma, [1] chroma
struct EncTables {
    unsigned short div[2][64];
    unsigned dc[2][16];
    unsigned ac[2][256];
};

constexpr EncTables make_tables() {
    EncTables t{};
    for (int c = 0; c < 2; ++c) {
        for (int i = 0; i < 64; ++i) {
            int q = (kStdQ[c][i] * 50 + 50) / 100;
            q = q < 1 ? 1 : (q > 255 ? 255 : q);
            t.div[c][i] = (unsigned short)(q << 3);
        }
        unsigned code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kDcCounts[c][len - 1]; ++i, ++code, ++k) t.dc[c][k] = code | ((unsigned)len << 16);   // symbols 0..11 in order
            code <<= 1;
        }
        code = 0; k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int i = 0; i < kAcCounts[c][len - 1]; ++i, ++code, ++k) t.ac[c][kAcSyms[c][k]] = code | ((unsigned)len << 16);
            code <<= 1;
        }
    }
    return t;
}

__constant__ EncTables kEnc = make_tables();

// ---- workspace: one image's geometry and, once the scans have run, where its streams lie
struct EncImg {
    long long rgb_off, block_base;        // bytes from `packed`; first block of the image among the batch's blocks
    int w, h, mcux, mcuy;
    unsigned long long nbytes;            // bytes of its bit stream before stuffing (the pad included)
    unsigned long long word0;             // first 32-bit word of that stream in the packed-word buffer
    unsigned long long out0, count;       // first byte and byte count of its stuffed scan in the output
};

struct EncHead {
    unsigned long long n_len;             // blocks + 1: elements of the length scan
    unsigned long long n_words;           // packed words in use: elements of the FF scan
};

struct EncLayout {                        // byte offsets into the workspace, each a multiple of 256
    long long blocks, cap_words;
    size_t head, tab, word0, ffbase, coefs, len, excl, tsum, words, fsum, total;
};

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

EncLayout enc_layout(long long blocks, int n) {
    EncLayout L{};
    L.blocks = blocks;
    L.cap_words = blocks * ENC_BLOCK_WORDS + n;
    size_t p = 0;
    L.head = p;   p += 256;
    L.tab = p;    p += up256(sizeof(EncImg) * (size_t)n);
    L.word0 = p;  p += up256(8 * ((size_t)n + 1));
    L.ffbase = p; p += up256(8 * ((size_t)n + 1));
    L.coefs = p;  p += up256(128 * (size_t)blocks);
    L.len = p;    p += up256(4 * ((size_t)blocks + 1));
    L.excl = p;   p += up256(8 * ((size_t)blocks + 1));
    L.tsum = p;   p += up256(8 * ((size_t)(blocks + 1 + ENC_TILE - 1) / ENC_TILE + 1));
    L.words = p;  p += up256(4 * (size_t)L.cap_words);
    L.fsum = p;   p += up256(8 * ((size_t)(L.cap_words + ENC_TILE - 1) / ENC_TILE + 1));
    L.total = p;
    return L;
}

struct EncChunk {
    long long rgb_off[ENC_CHUNK], block_base[ENC_CHUNK];
    int w[ENC_CHUNK], h[ENC_CHUNK];
    int first, count;
    unsigned long long n_len;
};

__global__ __launch_bounds__(64) void jpeg_enc_setup_kernel(EncChunk c, EncImg* __restrict__ tab, EncHead* __restrict__ head) {
    const int l = threadIdx.x;
    if (l < c.count) {
        EncImg im{};
        im.rgb_off = c.rgb_off[l]; im.block_base = c.block_base[l];
        im.w = c.w[l]; im.h = c.h[l];
        im.mcux = (c.w[l] + 15) >> 4; im.mcuy = (c.h[l] + 15) >> 4;
        tab[c.first + l] = im;
    }
    if (l == 0 && c.first == 0) { head->n_len = c.n_len; head->n_words = 0; }
}

// ---------------------------------------------------------------------------------------------------- front end
// jccolor.c rgb_ycc_convert, FIX(x) = int(x * 65536 + 0.5); comp 0 Y, 1 Cb, 2 Cr
__device__ __forceinline__ int ycc_of(const unsigned char* __restrict__ p, int comp) {
    const int r = p[0], g = p[1], b = p[2];
    if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// jfdctint.c jpeg_fdct_islow, one 1-D pass over eight values, in place (CONST_BITS 13, PASS1_BITS 2); 32-bit arithmetic is exact for
// 8-bit samples, as the IJG source notes.  first: the row pass (results scaled up by 4); else the column pass
template <bool first>
__device__ __forceinline__ void fdct_1d(int (&d)[8]) {
    constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299, F1847 = 15137,
                  F1961 = 16069, F2053 = 16819, F2562 = 20995, F3072 = 25172;
    constexpr int sh = first ? 13 - 2 : 13 + 2, rnd = 1 << (sh - 1);
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (first) { d[0] = (t10 + t11) << 2; d[4] = (t10 - t11) << 2; }
    else { d[0] = (t10 + t11 + 2) >> 2; d[4] = (t10 - t11 + 2) >> 2; }
    int z1 = (t12 + t13) * F0541;
    d[2] = (z1 + t13 * F0765 + rnd) >> sh;
    d[6] = (z1 - t12 * F1847 + rnd) >> sh;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * F1175;
    const int a4 = t4 * F0298, a5 = t5 * F2053, a6 = t6 * F3072, a7 = t7 * F1501;
    z1 *= -F0899; z2 *= -F2562; z3 = z3 * (-F1961) + z5; z4 = z4 * (-F0390) + z5;
    d[7] = (a4 + z1 + z3 + rnd) >> sh;
    d[5] = (a5 + z2 + z4 + rnd) >> sh;
    d[3] = (a6 + z2 + z3 + rnd) >> sh;
    d[1] = (a7 + z1 + z4 + rnd) >> sh;
}

// one thread = one block of image blockIdx.y, in scan order
__global__ __launch_bounds__(256) void jpeg_enc_fdct_kernel(const unsigned char* __restrict__ packed, const EncImg* __restrict__ tab,
                                                            short* __restrict__ coefs) {
    const EncImg im = tab[blockIdx.y];
    const long long nblk = 6ll * im.mcux * im.mcuy;
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= nblk) return;
    const long long mcu = b / 6;
    int k = (int)(b - mcu * 6);
    const int my = (int)(mcu / im.mcux), mx = (int)(mcu - (long long)my * im.mcux);
    const unsigned char* __restrict__ src = packed + im.rgb_off;
    const int w = im.w, h = im.h;
    int ws[8][8];
    bool dummy = false;
    if (k < 4) {
        // a luma block wholly beyond the image's block grid is not computed from padded pixels (jccoefct.c compress_data): AC 0,
        // DC that of the block before it in the MCU -- which is the nearest real one walking back, Y00 at the latest
        const int wb = (w + 7) >> 3, hb = (h + 7) >> 3;
        while (2 * mx + (k & 1) >= wb || 2 * my + (k >> 1) >= hb) { --k; dummy = true; }
        const int x0 = (2 * mx + (k & 1)) * 8, y0 = (2 * my + (k >> 1)) * 8;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int y = min(y0 + r, h - 1);                                  // the last real row / column replicated
            const unsigned char* __restrict__ row = src + (long long)y * w * 3;
#pragma unroll
            for (int c = 0; c < 8; ++c) ws[r][c] = ycc_of(row + 3 * min(x0 + c, w - 1), 0) - 128;
            fdct_1d<true>(ws[r]);
        }
    } else {
        // jcsample.c: the source columns replicated out to the MCU width, the source rows to an even count; then h2v2_downsample;
        // then the last DOWNSAMPLED row replicated down to the block height
        const int comp = k - 3, ch = (h + 1) >> 1;
        const int x0 = mx * 8, y0 = my * 8;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int cy = min(y0 + r, ch - 1);
            const unsigned char* __restrict__ ra = src + (long long)min(2 * cy, h - 1) * w * 3;
            const unsigned char* __restrict__ rb = src + (long long)min(2 * cy + 1, h - 1) * w * 3;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int xa = 3 * min(2 * (x0 + c), w - 1), xb = 3 * min(2 * (x0 + c) + 1, w - 1);
                const int s = ycc_of(ra + xa, comp) + ycc_of(ra + xb, comp) + ycc_of(rb + xa, comp) + ycc_of(rb + xb, comp);
                ws[r][c] = ((s + 1 + (c & 1)) >> 2) - 128;                     // bias 1, 2, 1, 2, ...
            }
            fdct_1d<true>(ws[r]);
        }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int col[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) col[r] = ws[r][c];
        fdct_1d<false>(col);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[r][c] = col[r];
    }
    // jcdctmgr.c: divisor q << 3 (the transform's output is scaled by 8), rounded half away from zero
    const unsigned short* __restrict__ div = kEnc.div[k < 4 ? 0 : 1];
    unsigned out[32];
#pragma unroll
    for (int p = 0; p < 64; ++p) {
        const int v = ws[kZig[p] >> 3][kZig[p] & 7];
        const unsigned d = div[kZig[p]];
        const unsigned a = ((unsigned)(v < 0 ? -v : v) + (d >> 1)) / d;
        int q = v < 0 ? -(int)a : (int)a;
        if (dummy && p > 0) q = 0;
        if (p & 1) out[p >> 1] |= (unsigned)(q & 0xFFFF) << 16;
        else out[p >> 1] = (unsigned)(q & 0xFFFF);
    }
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(coefs + (im.block_base + b) * 64);
#pragma unroll
    for (int i = 0; i < 8; ++i) dst[i] = make_uint4(out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]);
}

// ---------------------------------------------------------------------------------------------------- entropy coding
struct CountSink {
    unsigned bits = 0;
    __device__ __forceinline__ void put(unsigned, int n) { bits += n; }
};

// bits go out most significant first; `acc` holds the low `cnt` (< 32) pending bits, preceded by the zero bits of the word's head
// that belong to the block before
struct PackSink {
    unsigned* __restrict__ words;
    unsigned long long word;              // next word to write
    unsigned long long acc = 0;
    int cnt;
    bool first = true;
    __device__ __forceinline__ PackSink(unsigned* w, unsigned long long bitpos) : words(w), word(bitpos >> 5), cnt((int)(bitpos & 31)) {}
    __device__ __forceinline__ void put(unsigned code, int n) {
        acc = (acc << n) | code;
        cnt += n;
        if (cnt >= 32) {
            const unsigned v = __builtin_bswap32((unsigned)(acc >> (cnt - 32)));      // the stream is big-endian
            if (first) atomicOr(words + word, v);                                      // shared with the block before
            else words[word] = v;                                                      // all 32 bits are this block's
            first = false;
            ++word;
            cnt -= 32;
            acc &= (1ull << cnt) - 1ull;
        }
    }
    __device__ __forceinline__ void flush() {
        if (cnt > 0) atomicOr(words + word, __builtin_bswap32((unsigned)(acc << (32 - cnt))));   // shared with the block after
    }
};

__device__ __forceinline__ int nbits_of(int v) { return 32 - __clz(v < 0 ? -v : v); }     // __clz(0) = 32

// jchuff.c encode_one_block over the 64 zigzag-ordered coefficients at z, eight (one 16-byte load) at a time
template <class Sink>
__device__ __forceinline__ void encode_block(const uint4* __restrict__ z, int prev_dc, int tbl, Sink& s) {
    const unsigned* __restrict__ dct = kEnc.dc[tbl];
    const unsigned* __restrict__ act = kEnc.ac[tbl];
    int run = 0;
    for (int i = 0; i < 8; ++i) {
      const uint4 q = z[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned pair = (j >> 1) == 0 ? q.x : (j >> 1) == 1 ? q.y : (j >> 1) == 2 ? q.z : q.w;
        int c = (int)(short)((j & 1) ? (pair >> 16) : (pair & 0xFFFFu));
        if (i == 0 && j == 0) {
            c -= prev_dc;
            const int nb = nbits_of(c);
            const unsigned e = dct[nb];
            s.put(e & 0xFFFFu, (int)(e >> 16));
            if (nb) s.put((unsigned)(c < 0 ? c - 1 : c) & ((1u << nb) - 1u), nb);
            continue;
        }
        if (c == 0) { ++run; continue; }
        while (run > 15) { const unsigned e = act[0xF0]; s.put(e & 0xFFFFu, (int)(e >> 16)); run -= 16; }
        const int nb = nbits_of(c);
        const unsigned e = act[(run << 4) | nb];
        s.put(e & 0xFFFFu, (int)(e >> 16));
        s.put((unsigned)(c < 0 ? c - 1 : c) & ((1u << nb) - 1u), nb);
        run = 0;
      }
    }
    if (run > 0) { const unsigned e = act[0]; s.put(e & 0xFFFFu, (int)(e >> 16)); }
}

// block b of an image (scan order): its coefficients and the DC its difference is taken against (last_dc per component, 0 at
// the image's first MCU)
__device__ __forceinline__ void load_block(const short* __restrict__ coefs, long long g, long long b, const uint4*& z, int& prev_dc, int& tbl) {
    z = reinterpret_cast<const uint4*>(coefs + g * 64);
    const int k = (int)(b % 6);
    tbl = k < 4 ? 0 : 1;
    long long back = k == 0 ? 3 : (k < 4 ? 1 : 6);                     // Y00 follows the Y11 of the MCU before
    if (k >= 1 && k < 4) prev_dc = coefs[(g - 1) * 64];
    else prev_dc = b >= 6 ? coefs[(g - back) * 64] : 0;
}

__global__ __launch_bounds__(256) void jpeg_enc_len_kernel(const EncImg* __restrict__ tab, const short* __restrict__ coefs,
                                                           unsigned* __restrict__ len, int n) {
    const EncImg im = tab[blockIdx.y];
    const long long nblk = 6ll * im.mcux * im.mcuy;
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= nblk) return;
    const uint4* z;
    int prev_dc, tbl;
    load_block(coefs, im.block_base + b, b, z, prev_dc, tbl);
    CountSink s;
    encode_block(z, prev_dc, tbl, s);
    len[im.block_base + b] = s.bits;
    if ((int)blockIdx.y == n - 1 && b == nblk - 1) len[im.block_base + nblk] = 0;      // the scan's last element: its prefix is the total
}

__global__ __launch_bounds__(256) void jpeg_enc_pack_kernel(const EncImg* __restrict__ tab, const short* __restrict__ coefs,
                                                            const unsigned long long* __restrict__ excl, unsigned* __restrict__ words) {
    const EncImg im = tab[blockIdx.y];
    const long long nblk = 6ll * im.mcux * im.mcuy;
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= nblk) return;
    const uint4* z;
    int prev_dc, tbl;
    load_block(coefs, im.block_base + b, b, z, prev_dc, tbl);
    const unsigned long long start = excl[im.block_base];
    PackSink s(words, im.word0 * 32ull + (excl[im.block_base + b] - start));
    encode_block(z, prev_dc, tbl, s);
    if (b == nblk - 1) {                                               // jchuff.c flush_bits: the last byte filled with 1-bits
        const int r = (int)((excl[im.block_base + nblk] - start) & 7ull);
        if (r) s.put((1u << (8 - r)) - 1u, 8 - r);
    }
    s.flush();
}

// ---------------------------------------------------------------------------------------------------- prefix sums
__device__ __forceinline__ unsigned ff_count(unsigned x) {            // bytes of x equal to FF
    unsigned y = x & (x >> 4);
    y &= y >> 2;
    y &= y >> 1;
    return __popc(y & 0x01010101u);
}

struct LenLoad {
    const unsigned* __restrict__ p;
    __device__ __forceinline__ unsigned operator()(unsigned long long i) const { return p[i]; }
};
struct FfLoad {
    const unsigned* __restrict__ p;
    __device__ __forceinline__ unsigned operator()(unsigned long long i) const { return ff_count(p[i]); }
};

// exclusive prefix of v over the N threads of the workgroup; total: their sum.  (LDS, Hillis-Steele)
template <int N = 256>
__device__ __forceinline__ unsigned long long block_exclusive(unsigned long long v, unsigned long long& total) {
    __shared__ unsigned long long buf[2][N];
    const int t = threadIdx.x;
    int cur = 0;
    buf[0][t] = v;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < N; d <<= 1) {
        buf[cur ^ 1][t] = buf[cur][t] + (t >= d ? buf[cur][t - d] : 0ull);
        cur ^= 1;
        __syncthreads();
    }
    const unsigned long long incl = buf[cur][t];
    total = buf[cur][N - 1];
    __syncthreads();
    return incl - v;
}

// tile sums of load(0 .. *nptr - 1), tiles of ENC_TILE elements
template <class Load>
__global__ __launch_bounds__(256) void jpeg_enc_tile_sum_kernel(Load load, const unsigned long long* __restrict__ nptr,
                                                                unsigned long long* __restrict__ tsum) {
    const unsigned long long n = *nptr, ntiles = (n + ENC_TILE - 1) / ENC_TILE;
    for (unsigned long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        unsigned long long v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned long long i = t * ENC_TILE + threadIdx.x * 4 + j;
            if (i < n) v += load(i);
        }
        unsigned long long total;
        block_exclusive(v, total);
        if (threadIdx.x == 0) tsum[t] = total;
    }
}

// one workgroup: the tile sums -> their exclusive prefix, in place; tsum[ntiles] = the grand total
__global__ __launch_bounds__(256) void jpeg_enc_tile_scan_kernel(const unsigned long long* __restrict__ nptr,
                                                                 unsigned long long* __restrict__ tsum) {
    const unsigned long long n = *nptr, ntiles = (n + ENC_TILE - 1) / ENC_TILE;
    unsigned long long carry = 0;
    for (unsigned long long base = 0; base < ntiles; base += 256) {
        const unsigned long long i = base + threadIdx.x;
        const unsigned long long v = i < ntiles ? tsum[i] : 0ull;
        unsigned long long total;
        const unsigned long long ex = block_exclusive(v, total);
        if (i < ntiles) tsum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) tsum[ntiles] = carry;
}

__global__ __launch_bounds__(256) void jpeg_enc_len_scan_kernel(const unsigned* __restrict__ len, const unsigned long long* __restrict__ nptr,
                                                                const unsigned long long* __restrict__ tsum,
                                                                unsigned long long* __restrict__ excl) {
    const unsigned long long n = *nptr, ntiles = (n + ENC_TILE - 1) / ENC_TILE;
    for (unsigned long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const unsigned long long i0 = t * ENC_TILE + threadIdx.x * 4;
        unsigned v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i0 + j < n ? len[i0 + j] : 0u;
        unsigned long long total;
        unsigned long long run = tsum[t] + block_exclusive((unsigned long long)v[0] + v[1] + v[2] + v[3], total);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i0 + j < n) excl[i0 + j] = run;
            run += v[j];
        }
    }
}

// ---------------------------------------------------------------------------------------------------- layout and sizes
// per image: bytes of its bit stream (pad included) and its first packed word; the words in use
__global__ __launch_bounds__(64) void jpeg_enc_layout_kernel(EncImg* __restrict__ tab, int n, const unsigned long long* __restrict__ excl,
                                                             unsigned long long* __restrict__ word0, EncHead* __restrict__ head) {
    unsigned long long carry = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + (int)threadIdx.x;
        unsigned long long nbytes = 0;
        if (i < n) {
            const long long nblk = 6ll * tab[i].mcux * tab[i].mcuy;
            nbytes = (excl[tab[i].block_base + nblk] - excl[tab[i].block_base] + 7ull) >> 3;
        }
        unsigned long long total;
        const unsigned long long ex = block_exclusive<64>((nbytes + 3ull) >> 2, total);
        if (i < n) { tab[i].nbytes = nbytes; tab[i].word0 = carry + ex; word0[i] = carry + ex; }
        carry += total;
    }
    if (threadIdx.x == 0) { word0[n] = carry; head->n_words = carry; }
}

__global__ __launch_bounds__(256) void jpeg_enc_zero_kernel(unsigned* __restrict__ words, const EncHead* __restrict__ head) {
    const unsigned long long n = head->n_words;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) words[i] = 0u;
}

// ffbase[i], 0 <= i <= n: FF bytes in the packed words before word0[i] (one wave per i)
__global__ __launch_bounds__(256) void jpeg_enc_ffbase_kernel(const unsigned* __restrict__ words, const unsigned long long* __restrict__ word0,
                                                              const unsigned long long* __restrict__ fsum, int n,
                                                              unsigned long long* __restrict__ ffbase) {
    const int i = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i > n) return;
    const unsigned long long w0 = word0[i], t = w0 / ENC_TILE;
    unsigned c = 0;
    for (unsigned long long w = t * ENC_TILE + lane; w < w0; w += 64) c += ff_count(words[w]);
    c = fv_wave_sum(c);
    if (lane == 0) ffbase[i] = fsum[t] + c;
}

// per image: stuffed byte count and its place in the output, the scans back to back in image order
__global__ __launch_bounds__(64) void jpeg_enc_counts_kernel(EncImg* __restrict__ tab, int n, const unsigned long long* __restrict__ ffbase,
                                                             long long* __restrict__ counts) {
    unsigned long long carry = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + (int)threadIdx.x;
        const unsigned long long c = i < n ? tab[i].nbytes + (ffbase[i + 1] - ffbase[i]) : 0ull;
        unsigned long long total;
        const unsigned long long ex = block_exclusive<64>(c, total);
        if (i < n) { tab[i].count = c; tab[i].out0 = carry + ex; counts[i] = (long long)c; }
        carry += total;
    }
}

// ---------------------------------------------------------------------------------------------------- byte stuffing
// one thread = four packed words of a tile: every byte of theirs that belongs to a stream goes to its final place, a 00 behind
// every FF.  `limit` = the byte count the caller sized `out` for: nothing is written at or beyond it, whatever the tables say
__global__ __launch_bounds__(256) void jpeg_enc_stuff_kernel(const unsigned* __restrict__ words, const EncHead* __restrict__ head,
                                                             const EncImg* __restrict__ tab, const unsigned long long* __restrict__ word0,
                                                             const unsigned long long* __restrict__ ffbase,
                                                             const unsigned long long* __restrict__ fsum, int n,
                                                             unsigned char* __restrict__ out, unsigned long long limit) {
    const unsigned long long nw = head->n_words, ntiles = (nw + ENC_TILE - 1) / ENC_TILE;
    for (unsigned long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const unsigned long long w0 = t * ENC_TILE + threadIdx.x * 4;
        unsigned v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = w0 + j < nw ? words[w0 + j] : 0u;
        unsigned long long total;
        unsigned long long ff = fsum[t] + block_exclusive(ff_count(v[0]) + ff_count(v[1]) + ff_count(v[2]) + ff_count(v[3]), total);
        if (w0 >= nw) continue;
        int lo = 0, hi = n - 1;                                        // the image of word w0: the last i with word0[i] <= w0
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (word0[mid] <= w0) lo = mid; else hi = mid - 1;
        }
        int i = lo;
        unsigned long long next = word0[i + 1];
        EncImg im = tab[i];
        unsigned long long fb = ffbase[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned long long w = w0 + j;
            if (w >= nw) break;
            while (w >= next) { ++i; next = word0[i + 1]; im = tab[i]; fb = ffbase[i]; }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned long long p = (w - im.word0) * 4ull + k;           // byte of the image's unstuffed stream
                if (p >= im.nbytes) break;
                const unsigned byte = (v[j] >> (8 * k)) & 0xFFu;                   // memory order = stream order
                const unsigned long long o = im.out0 + p + (ff - fb);
                if (o < limit) out[o] = (unsigned char)byte;
                if (byte == 0xFFu) {
                    if (o + 1 < limit) out[o + 1] = 0;
                    ++ff;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------- host
struct EncPlan {
    long long blocks = 0, max_blocks = 0;
};

// 1 <= h, w <= 65535 for every image; -> false otherwise
bool enc_plan(const int32_t* hw, int n, EncPlan& P) {
    for (int i = 0; i < n; ++i) {
        const long long h = hw[2 * i], w = hw[2 * i + 1];
        if (h < 1 || w < 1 || h > 65535 || w > 65535) return false;
        const long long nb = 6 * ((w + 15) >> 4) * ((h + 15) >> 4);
        P.blocks += nb;
        if (nb > P.max_blocks) P.max_blocks = nb;
    }
    return true;
}

int enc_validate(fv_ctx* ctx, const char* who, const uint8_t* packed, int64_t packed_bytes, const int64_t* offsets, const int32_t* hw,
                 int n, void* workspace, size_t workspace_bytes, EncPlan& P, EncLayout& L) {
    FV_REQUIRE(ctx, packed && offsets && hw && workspace && packed_bytes >= 0 && n <= 65535, "%s: bad arguments (at most 65535 images)", who);
    FV_REQUIRE(ctx, enc_plan(hw, n, P), "%s: every image needs 1 <= rows, columns <= 65535", who);
    for (int i = 0; i < n; ++i)
        FV_REQUIRE(ctx, offsets[i] >= 0 && offsets[i] <= packed_bytes && 3ll * hw[2 * i] * hw[2 * i + 1] <= packed_bytes - offsets[i],
                   "%s: image %d (%d x %d at byte %lld) does not lie inside the %lld bytes of the buffer", who, i, hw[2 * i],
                   hw[2 * i + 1], (long long)offsets[i], (long long)packed_bytes);
    L = enc_layout(P.blocks, n);
    FV_REQUIRE(ctx, workspace_bytes >= L.total, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, L.total);
    FV_REQUIRE(ctx, ((uintptr_t)workspace & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
    return FV_OK;
}

template <class T>
inline T* at(void* ws, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }

inline unsigned capped(long long want, long long cap) { return (unsigned)(want < 1 ? 1 : (want > cap ? cap : want)); }

int enc_front_end(fv_ctx* ctx, const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n, void* ws, const EncPlan& P,
                  const EncLayout& L) {
    long long base = 0;
    for (int first = 0; first < n; first += ENC_CHUNK) {
        EncChunk c{};
        c.first = first; c.count = n - first < ENC_CHUNK ? n - first : ENC_CHUNK;
        c.n_len = (unsigned long long)P.blocks + 1ull;
        for (int l = 0; l < c.count; ++l) {
            const int i = first + l;
            c.rgb_off[l] = offsets[i]; c.block_base[l] = base;
            c.h[l] = hw[2 * i]; c.w[l] = hw[2 * i + 1];
            base += 6ll * ((hw[2 * i + 1] + 15) >> 4) * ((hw[2 * i] + 15) >> 4);
        }
        hipLaunchKernelGGL(jpeg_enc_setup_kernel, dim3(1), dim3(64), 0, ctx->stream, c, at<EncImg>(ws, L.tab), at<EncHead>(ws, L.head));
        FV_LAUNCH_CHECK(ctx);
    }
    FvProfScope ps(ctx, "jpeg_enc_fdct_kernel", 0.0, 0.0);
    hipLaunchKernelGGL(jpeg_enc_fdct_kernel, dim3((unsigned)((P.max_blocks + 255) / 256), (unsigned)n), dim3(256), 0, ctx->stream,
                       packed, at<EncImg>(ws, L.tab), at<short>(ws, L.coefs));
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}

}  // namespace

extern "C" {

int64_t fv_jpeg_encode_workspace_bytes(const int32_t* hw, int n) {
    EncPlan P;
    if (n < 0 || (n > 0 && !hw) || !enc_plan(hw, n, P)) return -1;
    return (int64_t)enc_layout(P.blocks, n).total;
}

int fv_jpeg_encode_coefs(fv_ctx* ctx, const uint8_t* packed, int64_t packed_bytes, const int64_t* offsets, const int32_t* hw, int n,
                         void* workspace, size_t workspace_bytes, int64_t* coef_offset_bytes) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, n >= 0, "jpeg_encode_coefs: n %d", n);
    if (n == 0) return FV_OK;
    EncPlan P;
    EncLayout L;
    if (int rc = enc_validate(ctx, "jpeg_encode_coefs", packed, packed_bytes, offsets, hw, n, workspace, workspace_bytes, P, L)) return rc;
    if (int rc = enc_front_end(ctx, packed, offsets, hw, n, workspace, P, L)) return rc;
    if (coef_offset_bytes) *coef_offset_bytes = (int64_t)L.coefs;
    return FV_OK;
}

int fv_jpeg_encode_measure(fv_ctx* ctx, const uint8_t* packed, int64_t packed_bytes, const int64_t* offsets, const int32_t* hw, int n,
                           void* workspace, size_t workspace_bytes, int64_t* counts) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, n >= 0, "jpeg_encode_measure: n %d", n);
    if (n == 0) return FV_OK;
    EncPlan P;
    EncLayout L;
    FV_REQUIRE(ctx, counts, "jpeg_encode_measure: bad arguments");
    if (int rc = enc_validate(ctx, "jpeg_encode_measure", packed, packed_bytes, offsets, hw, n, workspace, workspace_bytes, P, L)) return rc;
    if (int rc = enc_front_end(ctx, packed, offsets, hw, n, workspace, P, L)) return rc;
    void* ws = workspace;
    EncImg* tab = at<EncImg>(ws, L.tab);
    EncHead* head = at<EncHead>(ws, L.head);
    const short* coefs = at<short>(ws, L.coefs);
    unsigned* len = at<unsigned>(ws, L.len);
    unsigned long long* excl = at<unsigned long long>(ws, L.excl);
    unsigned long long* tsum = at<unsigned long long>(ws, L.tsum);
    unsigned long long* fsum = at<unsigned long long>(ws, L.fsum);
    unsigned long long* word0 = at<unsigned long long>(ws, L.word0);
    unsigned long long* ffbase = at<unsigned long long>(ws, L.ffbase);
    unsigned* words = at<unsigned>(ws, L.words);
    const dim3 per_block((unsigned)((P.max_blocks + 255) / 256), (unsigned)n);
    const unsigned len_tiles = capped((P.blocks + ENC_TILE) / ENC_TILE, 4096), word_tiles = capped((L.cap_words + ENC_TILE - 1) / ENC_TILE, 4096);
    {
        FvProfScope ps(ctx, "jpeg_enc_len_kernel", 0.0, 0.0);
        hipLaunchKernelGGL(jpeg_enc_len_kernel, per_block, dim3(256), 0, ctx->stream, tab, coefs, len, n);
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "jpeg_enc_len_scan", 0.0, 0.0);
        hipLaunchKernelGGL(jpeg_enc_tile_sum_kernel<LenLoad>, dim3(len_tiles), dim3(256), 0, ctx->stream, LenLoad{len}, &head->n_len, tsum);
        hipLaunchKernelGGL(jpeg_enc_tile_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, &head->n_len, tsum);
        hipLaunchKernelGGL(jpeg_enc_len_scan_kernel, dim3(len_tiles), dim3(256), 0, ctx->stream, len, &head->n_len, tsum, excl);
        hipLaunchKernelGGL(jpeg_enc_layout_kernel, dim3(1), dim3(64), 0, ctx->stream, tab, n, excl, word0, head);
        hipLaunchKernelGGL(jpeg_enc_zero_kernel, dim3(word_tiles), dim3(256), 0, ctx->stream, words, head);
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "jpeg_enc_pack_kernel", 0.0, 0.0);
        hipLaunchKernelGGL(jpeg_enc_pack_kernel, per_block, dim3(256), 0, ctx->stream, tab, coefs, excl, words);
        FV_LAUNCH_CHECK(ctx);
    }
    {
        FvProfScope ps(ctx, "jpeg_enc_ff_scan", 0.0, 0.0);
        hipLaunchKernelGGL(jpeg_enc_tile_sum_kernel<FfLoad>, dim3(word_tiles), dim3(256), 0, ctx->stream, FfLoad{words}, &head->n_words, fsum);
        hipLaunchKernelGGL(jpeg_enc_tile_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, &head->n_words, fsum);
        hipLaunchKernelGGL(jpeg_enc_ffbase_kernel, dim3((unsigned)(n / 4 + 1)), dim3(256), 0, ctx->stream, words, word0, fsum, n, ffbase);
        hipLaunchKernelGGL(jpeg_enc_counts_kernel, dim3(1), dim3(64), 0, ctx->stream, tab, n, ffbase, (long long*)counts);
        FV_LAUNCH_CHECK(ctx);
    }
    return FV_OK;
}

int fv_jpeg_encode_emit(fv_ctx* ctx, const int32_t* hw, int n, void* workspace, size_t workspace_bytes, const int64_t* counts,
                        uint8_t* out, int64_t out_bytes) {
    if (!ctx) return FV_ERR_INVALID;
    FV_REQUIRE(ctx, n >= 0, "jpeg_encode_emit: n %d", n);
    if (n == 0) return FV_OK;
    FV_REQUIRE(ctx, hw && workspace && counts && out && out_bytes >= 0 && n <= 65535, "jpeg_encode_emit: bad arguments");
    EncPlan P;
    FV_REQUIRE(ctx, enc_plan(hw, n, P), "jpeg_encode_emit: every image needs 1 <= rows, columns <= 65535");
    const EncLayout L = enc_layout(P.blocks, n);
    FV_REQUIRE(ctx, workspace_bytes >= L.total && ((uintptr_t)workspace & 15) == 0, "jpeg_encode_emit: workspace of %zu bytes, %zu needed",
               workspace_bytes, L.total);
    long long total = 0;
    for (int i = 0; i < n; ++i) {
        FV_REQUIRE(ctx, counts[i] >= 1 && counts[i] <= 2 * 4ll * ENC_BLOCK_WORDS * P.max_blocks + 8,
                   "jpeg_encode_emit: image %d: %lld bytes is no count fv_jpeg_encode_measure returns", i, (long long)counts[i]);
        total += counts[i];
    }
    FV_REQUIRE(ctx, total <= out_bytes, "jpeg_encode_emit: output of %lld bytes, %lld needed", (long long)out_bytes, total);
    void* ws = workspace;
    FvProfScope ps(ctx, "jpeg_enc_stuff_kernel", 0.0, (double)total);
    hipLaunchKernelGGL(jpeg_enc_stuff_kernel, dim3(capped((L.cap_words + ENC_TILE - 1) / ENC_TILE, 4096)), dim3(256), 0, ctx->stream,
                       at<unsigned>(ws, L.words), at<EncHead>(ws, L.head), at<EncImg>(ws, L.tab), at<unsigned long long>(ws, L.word0),
                       at<unsigned long long>(ws, L.ffbase), at<unsigned long long>(ws, L.fsum), n, out, (unsigned long long)total);
    FV_LAUNCH_CHECK(ctx);
    return FV_OK;
}

}  // extern "C"
