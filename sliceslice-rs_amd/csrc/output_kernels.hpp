// output_kernels.hpp - the kernels that write grep's output (include/sliceslice_hip_output.h; libsliceslice_hip_output.so only:
// ss_output.hip holds them and their host side).  The rule's arithmetic is output_host.hpp's, compiled here for the device.
//
//   output_sizes_kernel   one workgroup per block of SS_OUTPUT_BLOCK records, one lane per record and round, coalesced 8-byte loads:
//                         the bytes every record contributes (clamped text, terminator, digits, separator), summed in LDS, one
//                         8-byte store of the block's bytes.
//   prefix_kernel         (prefix_kernel.hpp) the bytes in front of every block, and their total.
//   output_starts_kernel  the sizes again, scanned inside the block in LDS; start[i] as 8 bytes per record, start[count] = the total.
//   output_copy_kernel    the grid is over the OUTPUT: one workgroup per chunk of SS_OUTPUT_CHUNK bytes, cut at multiples of that
//                         size from the 16-byte aligned address at or below d_out.  Two lanes find the records that hold the chunk's
//                         first and last byte by binary search in start[]; the workgroup stages runs of kOutputRun records (start,
//                         begin, length, number, what stands in front of the text) in LDS.  Every lane owns one 16-byte aligned unit
//                         of the output at a time, finds its record by binary search in the staged starts, and - the unit lies
//                         wholly inside that record's text - loads 16 bytes from the view, at whatever alignment they have there,
//                         and makes ONE 16-byte store.  A unit that holds a border, digits, a separator or a terminator is composed
//                         field by field in two 64-bit registers - a record's text by one 16-byte load wherever sixteen bytes of the
//                         view follow its first byte, the digits from the least significant one - and still stored once; only the
//                         units cut by d_out's own first and last byte are stored byte by byte.  A unit belongs to the run that holds its first byte; where it reaches beyond
//                         the run, the records behind come from global memory.
// Every output byte is stored exactly once.  A load from the view covers bytes of [b, e) of a clamped record only, so it touches no
// 16-byte block without a byte of the view.  No workgroup waits for another, no global atomic, the output depends on the input alone.
#pragma once
#include "output_launch.hpp"
#include "prefix_kernel.hpp"

#define SS_OUTPUT_FN __host__ __device__ __forceinline__
#include "output_host.hpp"

namespace ss {

constexpr uint32_t kOutBlock = SS_OUTPUT_BLOCK;
constexpr int kOutPer = (int)(kOutBlock / kOutputThreads);
constexpr uint32_t kOutChunk = SS_OUTPUT_CHUNK;
constexpr int kOutUnits = (int)(kOutChunk / 16 / kOutputCopyThreads);
static_assert(kOutBlock % kOutputThreads == 0 && kOutPer == 4, "a block is four records per lane");
static_assert(kOutChunk % (16 * kOutputCopyThreads) == 0 && kOutUnits == 4, "a chunk is four units per lane");
static_assert(kOutNumber == SS_OUTPUT_NUMBER && kOutSeparator == SS_OUTPUT_SEPARATOR, "output_host.hpp restates the header's flags");

// a record as the copy pass sees it
struct OutRecord {
    uint64_t b, tlen;           // its clamped text: hay[b, b + tlen)
    uint64_t number;
    uint32_t sep, num;          // the bytes of the separator and of the number in front of the text
    bool colon;                 // `:` behind the number, else `-`
};

// the number of entries of a[lo, hi) at or below x, plus lo
__device__ __forceinline__ uint64_t out_upper_bound(const uint64_t *a, uint64_t lo, uint64_t hi, uint64_t x)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint64_t out_prev_number(const OutputArgs &a, uint64_t i) { return (a.flags & kOutSeparator) && i != 0 ? a.number[i - 1] : 0; }

__device__ __forceinline__ uint64_t out_size_of(const OutputArgs &a, uint64_t i)
{
    return out_record_size(a.flags, a.terminator, i == 0, out_prev_number(a, i), a.flags ? a.number[i] : 0, a.begin[i], a.end[i], a.len);
}

__device__ __forceinline__ OutRecord out_load_record(const OutputArgs &a, uint64_t i)
{
    OutRecord r;
    uint64_t e;
    out_clamp(a.begin[i], a.end[i], a.len, &r.b, &e);
    r.tlen = e - r.b;
    r.number = a.flags ? a.number[i] : 0;
    const OutPrefix p = out_prefix(a.flags, a.terminator, i == 0, out_prev_number(a, i), r.number);
    r.sep = p.sep;
    r.num = p.num;
    r.colon = !a.kind || a.kind[i] != 0;
    return r;
}

__global__ void __launch_bounds__(kOutputThreads) output_sizes_kernel(OutputArgs a)
{
    __shared__ uint64_t s_sum[kOutputThreads];
    const uint64_t base = (uint64_t)blockIdx.x * kOutBlock;
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kOutPer; ++k) {
        const uint64_t i = base + threadIdx.x + (uint64_t)k * kOutputThreads;
        if (i < a.count) sum += out_size_of(a, i);
    }
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (unsigned k = kOutputThreads / 2; k != 0; k >>= 1) {
        if (threadIdx.x < k) s_sum[threadIdx.x] += s_sum[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.sum[blockIdx.x] = s_sum[0];
}

__global__ void __launch_bounds__(kOutputThreads) output_starts_kernel(OutputArgs a)
{
    __shared__ uint64_t s_size[kOutBlock];
    __shared__ uint64_t s_run[kOutputThreads];
    const uint64_t base = (uint64_t)blockIdx.x * kOutBlock;
    const uint32_t n = a.count - base < kOutBlock ? (uint32_t)(a.count - base) : kOutBlock;
#pragma unroll
    for (int k = 0; k < kOutPer; ++k) {
        const uint32_t j = threadIdx.x + (uint32_t)k * kOutputThreads;
        s_size[j] = j < n ? out_size_of(a, base + j) : 0;
    }
    __syncthreads();
    // lane t owns the sizes kOutPer * t ..; the lanes' sums are scanned (Hillis-Steele, inclusive), then every lane ranks its own
    uint64_t v[kOutPer], sum = 0;
#pragma unroll
    for (int k = 0; k < kOutPer; ++k) {
        v[k] = s_size[threadIdx.x * kOutPer + k];
        sum += v[k];
    }
    s_run[threadIdx.x] = sum;
    __syncthreads();
    for (int k = 1; k < kOutputThreads; k <<= 1) {
        const uint64_t w = threadIdx.x >= (unsigned)k ? s_run[threadIdx.x - k] : 0ull;
        __syncthreads();
        s_run[threadIdx.x] += w;
        __syncthreads();
    }
    uint64_t r = s_run[threadIdx.x] - sum;
#pragma unroll
    for (int k = 0; k < kOutPer; ++k) {
        s_size[threadIdx.x * kOutPer + k] = r;
        r += v[k];
    }
    __syncthreads();
    const uint64_t rank = a.rank[blockIdx.x];
#pragma unroll
    for (int k = 0; k < kOutPer; ++k) {
        const uint32_t j = threadIdx.x + (uint32_t)k * kOutputThreads;
        if (j < n) a.starts[base + j] = rank + s_size[j];
    }
    if (blockIdx.x == a.blocks - 1 && threadIdx.x == kOutputThreads - 1) a.starts[a.count] = rank + s_run[threadIdx.x];
}

// 16 bytes of the view at any alignment, every one of them a byte of the view.
#ifndef SS_OUTPUT_ALIGNED_PAIR
// One global load: the target allows unaligned vector accesses.
typedef uint32_t out_u32x4_unaligned __attribute__((ext_vector_type(4), aligned(1)));
__device__ __forceinline__ uint4 out_load16(const uint8_t *src)
{
    const out_u32x4_unaligned v = *reinterpret_cast<const out_u32x4_unaligned *>(src);
    return make_uint4(v.x, v.y, v.z, v.w);
}
#else
// The alternative that was measured against it (an A/B build with -DSS_OUTPUT_ALIGNED_PAIR=1): the two aligned
// blocks that hold the bytes, shifted together.  The second block is loaded only where the source is misaligned: it then holds the
// last of the sixteen bytes, so it is no block without a byte of the view.
__device__ __forceinline__ uint4 out_load16(const uint8_t *src)
{
    const unsigned sh = (unsigned)(reinterpret_cast<uintptr_t>(src) & 15);
    const uint4 *p = reinterpret_cast<const uint4 *>(src - sh);
    const uint4 lo = p[0];
    if (sh == 0) return lo;
    const uint4 hi = p[1];
    uint64_t w0 = lo.x | (uint64_t)lo.y << 32, w1 = lo.z | (uint64_t)lo.w << 32;
    uint64_t w2 = hi.x | (uint64_t)hi.y << 32;
    const uint64_t w3 = hi.z | (uint64_t)hi.w << 32;
    if (sh >= 8) {
        w0 = w1;
        w1 = w2;
        w2 = w3;
    }
    const unsigned s = (sh & 7) * 8;
    if (s != 0) {
        w0 = w0 >> s | w1 << (64 - s);
        w1 = w1 >> s | w2 << (64 - s);
    }
    return make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
}
#endif

// byte `t` (0 .. 15) of the unit held in (w0, w1)
__device__ __forceinline__ void out_put(uint64_t &w0, uint64_t &w1, unsigned t, uint8_t byte)
{
    if (t < 8) w0 |= (uint64_t)byte << (8 * t);
    else w1 |= (uint64_t)byte << (8 * (t - 8));
}

// the first m (1 .. 16 - t) bytes of v at the bytes t .. of the unit
__device__ __forceinline__ void out_put_bytes(uint64_t &w0, uint64_t &w1, unsigned t, unsigned m, uint4 v)
{
    uint64_t v0 = v.x | (uint64_t)v.y << 32, v1 = v.z | (uint64_t)v.w << 32;
    if (m < 8) {
        v0 &= (1ull << (8 * m)) - 1;
        v1 = 0;
    } else if (m < 16) {
        v1 &= (1ull << (8 * (m - 8))) - 1;
    }
    if (t >= 8) {
        v1 = v0 << (8 * (t - 8));
        v0 = 0;
    } else if (t != 0) {
        v1 = v1 << (8 * t) | v0 >> (64 - 8 * t);
        v0 <<= 8 * t;
    }
    w0 |= v0;
    w1 |= v1;
}

__global__ void __launch_bounds__(kOutputCopyThreads) output_copy_kernel(OutputArgs a)
{
    __shared__ uint64_t s_start[kOutputRun + 1], s_b[kOutputRun], s_tlen[kOutputRun], s_number[kOutputRun];
    __shared__ uint8_t s_meta[kOutputRun];                              // sep | num << 2 | colon << 7
    __shared__ uint64_t s_slice[2];
    const uint64_t q0 = (uint64_t)blockIdx.x * kOutChunk;
    const uint64_t qlo = q0 > a.out_lo ? q0 : a.out_lo, qhi = q0 + kOutChunk < a.out_hi ? q0 + kOutChunk : a.out_hi;
    if (qlo >= qhi) return;                                             // (workgroup-uniform; the host launches no such chunk)
    if (threadIdx.x < 2) {
        // the last record that begins at or below the chunk's first byte - the records of its start in front of it are empty - and
        // the one that holds the chunk's last byte
        const uint64_t o = (threadIdx.x == 0 ? qlo : qhi - 1) - a.out_lo;
        const uint64_t k = out_upper_bound(a.starts, 0, a.count, o);
        s_slice[threadIdx.x] = k != 0 ? k - 1 : 0;
    }
    __syncthreads();
    const uint64_t r0 = s_slice[0], r1 = s_slice[1];
    const uint8_t term = (uint8_t)a.terminator;
    for (uint64_t rs = r0; rs <= r1; rs += kOutputRun) {
        const uint32_t n = r1 - rs + 1 < kOutputRun ? (uint32_t)(r1 - rs + 1) : kOutputRun;
        if (rs != r0) __syncthreads();                                  // (the run before has been read)
        for (uint32_t j = threadIdx.x; j <= n; j += kOutputCopyThreads) s_start[j] = a.starts[rs + j];
        for (uint32_t j = threadIdx.x; j < n; j += kOutputCopyThreads) {
            const OutRecord r = out_load_record(a, rs + j);
            s_b[j] = r.b;
            s_tlen[j] = r.tlen;
            s_number[j] = r.number;
            s_meta[j] = (uint8_t)(r.sep | r.num << 2 | (r.colon ? 0x80u : 0u));
        }
        __syncthreads();
        const uint64_t run_lo = s_start[0], run_hi = s_start[n];
#pragma unroll 1
        for (int k = 0; k < kOutUnits; ++k) {
            const uint64_t u = q0 + ((uint64_t)threadIdx.x + (uint64_t)k * kOutputCopyThreads) * 16;
            const uint64_t lo = u > qlo ? u : qlo, hi = u + 16 < qhi ? u + 16 : qhi;
            if (lo >= hi) continue;
            const uint64_t o = lo - a.out_lo;
            if (o < run_lo || o >= run_hi) continue;                    // (another run's unit)
            // the staged record that holds byte o: the last one that begins at or below it
            uint32_t l = 0, h = n;
            while (l < h) {
                const uint32_t mid = l + (h - l) / 2;
                if (s_start[mid] <= o) l = mid + 1;
                else h = mid;
            }
            uint32_t li = l - 1;                                        // (s_start[0] <= o)
            OutRecord r;
            r.b = s_b[li];
            r.tlen = s_tlen[li];
            r.number = s_number[li];
            r.sep = s_meta[li] & 3u;
            r.num = (s_meta[li] >> 2) & 31u;
            r.colon = (s_meta[li] & 0x80u) != 0;
            uint64_t st = s_start[li], nxt = s_start[li + 1];
            const uint64_t text = st + r.sep + r.num;
            const bool whole = hi - lo == 16;
            if (whole && o >= text && o - text + 16 <= r.tlen) {
                *reinterpret_cast<uint4 *>(a.out_base + u) = out_load16(a.hay + r.b + (o - text));
                continue;
            }
            uint64_t i = rs + li, w0 = 0, w1 = 0, q = lo;
            while (q < hi) {                                            // field by field: each adds at least one byte
                const uint64_t oo = q - a.out_lo;
                while (oo >= nxt && i + 1 < a.count) {                  // the next record that holds a byte
                    ++i;
                    const uint64_t lj = i - rs;
                    st = nxt;
                    if (lj < n) {
                        r.b = s_b[lj];
                        r.tlen = s_tlen[lj];
                        r.number = s_number[lj];
                        r.sep = s_meta[lj] & 3u;
                        r.num = (s_meta[lj] >> 2) & 31u;
                        r.colon = (s_meta[lj] & 0x80u) != 0;
                        nxt = s_start[lj + 1];
                    } else {
                        r = out_load_record(a, i);
                        nxt = a.starts[i + 1];
                    }
                }
                const unsigned t = (unsigned)(q - u), room = (unsigned)(hi - q);
                uint64_t off = oo - st;
                if (off < r.sep) {
                    out_put(w0, w1, t, off < 2 ? (uint8_t)'-' : term);
                    ++q;
                } else if ((off -= r.sep) < r.num) {
                    // the digits from the least significant one, behind them `:` or `-`; those of [k, k + m) lie in the unit
                    const unsigned k = (unsigned)off, m = r.num - k < room ? r.num - k : room;
                    uint64_t v = r.number;
                    for (unsigned p = r.num - 1;; --p) {
                        uint8_t byte = (uint8_t)(r.colon ? ':' : '-');
                        if (p != r.num - 1) {
                            byte = (uint8_t)('0' + v % 10u);
                            v /= 10u;
                        }
                        if (p < k + m) out_put(w0, w1, t + (p - k), byte);
                        if (p == k) break;
                    }
                    q += m;
                } else if ((off -= r.num) < r.tlen) {
                    const unsigned m = r.tlen - off < room ? (unsigned)(r.tlen - off) : room;
                    const uint64_t src = r.b + off;
                    if (src + 16 <= a.len) {                            // sixteen bytes of the view, the first m of them the record's
                        out_put_bytes(w0, w1, t, m, out_load16(a.hay + src));
                    } else {
                        for (unsigned j = 0; j < m; ++j) out_put(w0, w1, t + j, a.hay[src + j]);
                    }
                    q += m;
                } else {
                    out_put(w0, w1, t, term);
                    ++q;
                }
            }
            if (whole) {
                *reinterpret_cast<uint4 *>(a.out_base + u) = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
            } else {
                for (uint64_t q = lo; q < hi; ++q) {                    // a unit cut by d_out's own first or last byte
                    const unsigned t = (unsigned)(q - u);
                    a.out_base[q] = (uint8_t)((t < 8 ? w0 : w1) >> (8 * (t & 7)));
                }
            }
        }
    }
}

}  // namespace ss
