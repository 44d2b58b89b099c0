// json_sync.hip — nidx_gpu_json_sync on the device (gfx950, wave64): the open JSON index moves to the shard's next generation without
// a per-document datum of a kept segment crossing the bus.  The host (json_index.cpp, planned by json_sync_plan.h) hands over one table
// row per entry of the new generation (its first word in the old rows, or none for a new segment; its seq) and the new word offsets;
// every kernel finds its entry in those tables, so the number of launches depends neither on the kept segments nor on the deletions:
//   mark    json_sync_mark_rows_kernel: the old ordinals the kept segments' documents name -> bits of `used`
//           json_sync_mark_ids_kernel:  the new documents' uuids the old table holds (json_link_kernel found them) -> bits of `used`
//   rank    json_sync_rank_kernel: the exclusive running count of used bits per word (one workgroup; the table is small)
//   table   json_sync_table_kernel: the new table = the merge by rank of the survivors (the old table compacted by `used`) and the
//           uuids only new documents name; remap[old ordinal] = new ordinal or UINT32_MAX; del_seq starts at "no deletion"
//   dels    json_sync_deletions_kernel: every distinct deletion the new table holds writes its seq into its own slot of del_seq
//   carry   json_sync_carry_kernel: a kept segment's ordinals through remap to its new word offset, every entry's alive words minus
//           the ballot of del_seq[resource] > seq(entry); the cleared bits are counted
// Plain loads, vector stores and atomics only.
#include <limits.h>

#include "device_common.h"
#include "json_sync_plan.h"
#include "kernels.h"

namespace nidx {

namespace {
// the first index of table[n][2] (ascending, first word major) that is not below (hi, lo)
__device__ __forceinline__ uint32_t json_sync_lower_bound(const uint64_t *__restrict__ table, uint32_t n, uint64_t hi, uint64_t lo) {
    uint32_t a = 0, b = n;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        const uint64_t th = table[2 * (size_t)mid], tl = table[2 * (size_t)mid + 1];
        if (th < hi || (th == hi && tl < lo)) a = mid + 1;
        else b = mid;
    }
    return a;
}

// the entry that owns word w of the new rows: the last e with word0[e] <= w (an empty entry owns no word); w < word0[n_entries]
__device__ __forceinline__ uint32_t json_sync_entry_of(const uint64_t *__restrict__ word0, uint32_t n_entries, uint64_t w) {
    uint32_t a = 0, b = n_entries;   // the first e in [0, n_entries] with word0[e] > w, minus one
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2;
        if (word0[mid] <= w) a = mid + 1;
        else b = mid;
    }
    return a - 1u;   // (word0[0] = 0 <= w: a >= 1)
}
}  // namespace

// grid = 64-word spans of the NEW rows, one wave per span (as json_resource_rows_kernel); a lane per document of the word.
__global__ __launch_bounds__(256) void json_sync_mark_rows_kernel(const uint64_t *__restrict__ word0, const JsonSyncRow *__restrict__ rows,
                                                                  uint32_t n_entries, uint64_t n_words,
                                                                  const uint32_t *__restrict__ old_doc_resource, uint32_t n_old_resources,
                                                                  unsigned long long *__restrict__ used) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t w_begin = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u;
    if (w_begin >= n_words) return;   // (uniform per wave)
    const uint64_t w_end = w_begin + 64u < n_words ? w_begin + 64u : n_words;
    uint32_t e = json_sync_entry_of(word0, n_entries, w_begin);
    for (uint64_t w = w_begin; w < w_end; w++) {   // uniform per wave
        while (w >= word0[e + 1]) e++;
        const uint64_t ow0 = rows[e].old_word0;
        if (ow0 == kJsonSyncNew) continue;
        const uint32_t r = old_doc_resource[(ow0 + (w - word0[e])) * 64u + lane];
        if (r < n_old_resources) atomicOr(&used[r >> 6], 1ull << (r & 63u));
    }
}

__global__ __launch_bounds__(256) void json_sync_mark_ids_kernel(const uint32_t *__restrict__ found, uint32_t n, uint32_t n_old_resources,
                                                                 unsigned long long *__restrict__ used) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = found[i];
    if (r < n_old_resources) atomicOr(&used[r >> 6], 1ull << (r & 63u));
}

// word_rank[w] = the used bits in the words below w, for w in [0, n); *n_used = all of them.  One workgroup: a thread sums a contiguous
// chunk of words, the 256 sums are scanned in LDS, the thread writes its chunk's running counts.
__global__ __launch_bounds__(256) void json_sync_rank_kernel(const unsigned long long *__restrict__ used, uint32_t n, uint32_t *__restrict__ word_rank,
                                                             unsigned long long *__restrict__ n_used) {
    __shared__ uint32_t part[256];
    const uint32_t t = threadIdx.x, chunk = (n + 255u) / 256u;
    const uint32_t w0 = t * chunk < n ? t * chunk : n, w1 = w0 + chunk < n ? w0 + chunk : n;
    uint32_t sum = 0;
    for (uint32_t w = w0; w < w1; w++) sum += (uint32_t)__popcll(used[w]);
    part[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 256u; off <<= 1) {
        const uint32_t v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (uint32_t w = w0; w < w1; w++) {
        word_rank[w] = run;
        run += (uint32_t)__popcll(used[w]);
    }
    if (t == 255u) *n_used = part[255];
}

// One thread per old ordinal and per new-only uuid.  `used` and word_rank hold one word more than the old table needs, so that the rank
// of "past the end" is read like any other.
__global__ __launch_bounds__(256) void json_sync_table_kernel(const uint64_t *__restrict__ old_table, uint32_t n_old,
                                                              const unsigned long long *__restrict__ used, const uint32_t *__restrict__ word_rank,
                                                              const uint64_t *__restrict__ new_only, uint32_t n_new_only,
                                                              uint64_t *__restrict__ new_table, uint32_t *__restrict__ remap,
                                                              long long *__restrict__ del_seq) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)n_old + n_new_only) return;
    uint64_t hi, lo;
    uint32_t pos;
    if (i < n_old) {
        const uint32_t r = (uint32_t)i;
        const unsigned long long uw = used[r >> 6];
        if (!((uw >> (r & 63u)) & 1ull)) {
            remap[r] = 0xffffffffu;
            return;
        }
        hi = old_table[2 * (size_t)r], lo = old_table[2 * (size_t)r + 1];
        pos = word_rank[r >> 6] + (uint32_t)__popcll(uw & ((1ull << (r & 63u)) - 1ull)) + json_sync_lower_bound(new_only, n_new_only, hi, lo);
        remap[r] = pos;
    } else {
        const uint32_t j = (uint32_t)(i - n_old);
        hi = new_only[2 * (size_t)j], lo = new_only[2 * (size_t)j + 1];
        const uint32_t lb = json_sync_lower_bound(old_table, n_old, hi, lo);   // (the old table does not hold it)
        pos = j + word_rank[lb >> 6] + (uint32_t)__popcll(used[lb >> 6] & ((1ull << (lb & 63u)) - 1ull));
    }
    new_table[2 * (size_t)pos] = hi;
    new_table[2 * (size_t)pos + 1] = lo;
    del_seq[pos] = LLONG_MIN;   // no deletion names it (every new ordinal is written by exactly one thread)
}

// ordinals[i] = the new ordinal of distinct deletion i (UINT32_MAX: the table does not hold it): each writes its own slot
__global__ __launch_bounds__(256) void json_sync_deletions_kernel(const uint32_t *__restrict__ ordinals, const long long *__restrict__ seqs, uint32_t n,
                                                                  uint32_t n_resources, long long *__restrict__ del_seq) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = ordinals[i];
    if (r < n_resources) del_seq[r] = seqs[i];
}

// grid as json_sync_mark_rows_kernel.  A kept entry's word comes from the old rows, its ordinals go through remap (padding stays
// UINT32_MAX); a new entry's word and ordinals are already in place (uploaded, and linked over the new table).  Every lane then asks
// whether a deletion newer than the entry names its document's resource; the ballot leaves the alive word.
__global__ __launch_bounds__(256) void json_sync_carry_kernel(const uint64_t *__restrict__ word0, const JsonSyncRow *__restrict__ rows, uint32_t n_entries,
                                                              uint64_t n_words, const uint64_t *__restrict__ old_alive,
                                                              const uint32_t *__restrict__ old_doc_resource, const uint32_t *__restrict__ remap,
                                                              uint32_t n_old_resources, const long long *__restrict__ del_seq, uint32_t n_resources,
                                                              uint64_t *new_alive, uint32_t *new_doc_resource, unsigned long long *__restrict__ cleared) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t w_begin = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u;
    if (w_begin >= n_words) return;   // (uniform per wave)
    const uint64_t w_end = w_begin + 64u < n_words ? w_begin + 64u : n_words;
    uint32_t e = json_sync_entry_of(word0, n_entries, w_begin);
    unsigned long long c = 0;
    for (uint64_t w = w_begin; w < w_end; w++) {   // uniform per wave
        while (w >= word0[e + 1]) e++;
        const JsonSyncRow row = rows[e];
        uint64_t a;
        uint32_t r;
        if (row.old_word0 != kJsonSyncNew) {
            const uint64_t ow = row.old_word0 + (w - word0[e]);
            a = old_alive[ow];
            const uint32_t ro = old_doc_resource[ow * 64u + lane];
            r = ro < n_old_resources ? remap[ro] : 0xffffffffu;
            new_doc_resource[w * 64u + lane] = r;
        } else {
            a = new_alive[w];
            r = new_doc_resource[w * 64u + lane];
        }
        const bool deleted = r < n_resources && del_seq[r] > (long long)row.seq;
        const unsigned long long clear = __ballot(deleted) & a;
        if (lane == 0u) {
            new_alive[w] = a & ~clear;
            c += (unsigned long long)__popcll(clear);
        }
    }
    if (lane == 0u && c) atomicAdd(cleared, c);
}

static uint32_t json_sync_span_blocks(uint64_t n_words) { return (uint32_t)(((n_words + 63) / 64 + 3) / 4); }

hipError_t launch_json_sync_mark_rows(const uint64_t *word0, const JsonSyncRow *rows, uint32_t n_entries, uint64_t n_words,
                                      const uint32_t *old_doc_resource, uint32_t n_old_resources, unsigned long long *used, hipStream_t s) {
    if (!n_words || !n_entries) return hipSuccess;
    hipLaunchKernelGGL(json_sync_mark_rows_kernel, dim3(json_sync_span_blocks(n_words)), dim3(256), 0, s, word0, rows, n_entries, n_words, old_doc_resource,
                       n_old_resources, used);
    return hipGetLastError();
}

hipError_t launch_json_sync_mark_ids(const uint32_t *found, uint32_t n, uint32_t n_old_resources, unsigned long long *used, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(json_sync_mark_ids_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, found, n, n_old_resources, used);
    return hipGetLastError();
}

hipError_t launch_json_sync_rank(const unsigned long long *used, uint32_t n_words, uint32_t *word_rank, unsigned long long *n_used, hipStream_t s) {
    hipLaunchKernelGGL(json_sync_rank_kernel, dim3(1), dim3(256), 0, s, used, n_words, word_rank, n_used);
    return hipGetLastError();
}

hipError_t launch_json_sync_table(const uint64_t *old_table, uint32_t n_old, const unsigned long long *used, const uint32_t *word_rank,
                                  const uint64_t *new_only, uint32_t n_new_only, uint64_t *new_table, uint32_t *remap, long long *del_seq,
                                  hipStream_t s) {
    const uint64_t n = (uint64_t)n_old + n_new_only;
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(json_sync_table_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, old_table, n_old, used, word_rank, new_only, n_new_only,
                       new_table, remap, del_seq);
    return hipGetLastError();
}

hipError_t launch_json_sync_deletions(const uint32_t *ordinals, const long long *seqs, uint32_t n, uint32_t n_resources, long long *del_seq,
                                      hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(json_sync_deletions_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, ordinals, seqs, n, n_resources, del_seq);
    return hipGetLastError();
}

hipError_t launch_json_sync_carry(const uint64_t *word0, const JsonSyncRow *rows, uint32_t n_entries, uint64_t n_words, const uint64_t *old_alive,
                                  const uint32_t *old_doc_resource, const uint32_t *remap, uint32_t n_old_resources, const long long *del_seq,
                                  uint32_t n_resources, uint64_t *new_alive, uint32_t *new_doc_resource, unsigned long long *cleared,
                                  hipStream_t s) {
    if (!n_words || !n_entries) return hipSuccess;
    hipLaunchKernelGGL(json_sync_carry_kernel, dim3(json_sync_span_blocks(n_words)), dim3(256), 0, s, word0, rows, n_entries, n_words, old_alive,
                       old_doc_resource, remap, n_old_resources, del_seq, n_resources, new_alive, new_doc_resource, cleared);
    return hipGetLastError();
}

}  // namespace nidx
