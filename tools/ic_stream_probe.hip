// ic_stream_probe.hip — what the 256 MiB Infinity Cache keeps of the partition's intermediates between two passes.
//   hipcc --offload-arch=gfx950 -O3 -o ic_stream_probe tools/ic_stream_probe.hip && timeout 60 ./ic_stream_probe > profiles/r08_ic_probe.json
// Stand-alone (no libgndt, no torch).  Streaming kernels, 16 bytes per lane, at the sizes of the bench scene (10 M points): the cloud is
// 120 MB, recs1 / recs are 160 MB each.  Every case is run kReps times behind a 512 MB scrub read; the JSON carries the median rate of
// the timed kernel in TB/s.  A timed figure is ONE kernel of 25-55 us between two hipEventRecord calls: the events' own few microseconds
// are inside every rate, so the absolute TB/s are lower bounds; the comparisons between cases are what the probe is for.
//   (a) write 160 MB, read it back                                   — the resident case; "cold": the read behind the scrub alone
//   (b) write 160 MB, read 120 MB and then 160 MB of OTHER buffers, read the first back — the in-between reads plain | non-temporal
//   (c) a producer reads 160 MB and writes 160 MB in 53 slabs (level 2's shape: blockIdx.y is the slab), a consumer reads what it
//       wrote slab by slab, ascending | descending; the producer's loads plain | non-temporal
//   (p) the partition's chain: 120 MB -> 160 MB (level 1), 160 MB -> 160 MB in slabs (level 2), consumer (bucket kernel): loads of the
//       two copies plain | non-temporal, consumer ascending | descending; level 2's and the consumer's rates
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef float f4 __attribute__((ext_vector_type(4)));

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

constexpr int kT = 256, kPer = 4, kReps = 9;
constexpr uint32_t kSlabs = 53;

template <bool NT>
__device__ __forceinline__ f4 ld(const f4* p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

__global__ void __launch_bounds__(kT) k_write(f4* __restrict__ dst, uint32_t n) {
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const uint32_t i = (blockIdx.x * kPer + j) * kT + threadIdx.x;
        if (i < n) dst[i] = f4{1.f, 2.f, 3.f, (float)(i & 1023u)};
    }
}

template <bool NT>
__global__ void __launch_bounds__(kT) k_read(const f4* __restrict__ src, uint32_t n, f4* __restrict__ sink) {
    f4 v[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const uint32_t i = (blockIdx.x * kPer + j) * kT + threadIdx.x;
        v[j] = i < n ? ld<NT>(src + i) : f4{0.f, 0.f, 0.f, 0.f};
    }
    f4 s = v[0];
#pragma unroll
    for (int j = 1; j < kPer; ++j) s += v[j];
    if (s.x == -1.f) sink[0] = s;          // (never: the buffers hold positive values)
}

template <bool NT>
__global__ void __launch_bounds__(kT) k_copy(const f4* __restrict__ src, uint32_t n_src, f4* __restrict__ dst, uint32_t n_dst) {
    // n_dst elements written: element i is src[i] for i < n_src and a constant behind it (a 120 MB source, a 160 MB destination)
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const uint32_t i = (blockIdx.x * kPer + j) * kT + threadIdx.x;
        if (i < n_dst) {
            f4 v = f4{1.f, 1.f, 1.f, 1.f};
            if (i < n_src) v = ld<NT>(src + i);
            dst[i] = v;
        }
    }
}

// slab blockIdx.y (or the mirror of it) of n elements cut into kSlabs: copy, or read
template <bool NT>
__global__ void __launch_bounds__(kT) k_slab_copy(const f4* __restrict__ src, f4* __restrict__ dst, uint32_t n, uint32_t per_slab) {
    const uint32_t s0 = blockIdx.y * per_slab, s1 = min(s0 + per_slab, n);
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const uint32_t i = s0 + (blockIdx.x * kPer + j) * kT + threadIdx.x;
        if (i < s1) dst[i] = ld<NT>(src + i);
    }
}
template <bool NT>
__global__ void __launch_bounds__(kT) k_slab_read(const f4* __restrict__ src, uint32_t n, uint32_t per_slab, uint32_t reverse, f4* __restrict__ sink) {
    const uint32_t slab = reverse ? gridDim.y - 1u - blockIdx.y : blockIdx.y;
    const uint32_t s0 = slab * per_slab, s1 = min(s0 + per_slab, n);
    f4 s = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const uint32_t i = s0 + (blockIdx.x * kPer + j) * kT + threadIdx.x;
        if (i < s1) s += ld<NT>(src + i);
    }
    if (s.x == -1.f) sink[0] = s;
}

static uint32_t blocks(uint32_t n) { return (n + kT * kPer - 1) / (kT * kPer); }

struct Timer {
    hipEvent_t a, b;
    Timer() { CK(hipEventCreate(&a)); CK(hipEventCreate(&b)); }
    void start() { CK(hipEventRecord(a, 0)); }
    double stop_us() { CK(hipEventRecord(b, 0)); CK(hipEventSynchronize(b)); float ms = 0.f; CK(hipEventElapsedTime(&ms, a, b)); return 1e3 * (double)ms; }
};

static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
static double tbs(double bytes, double us) { return bytes / us * 1e-6; }

int main() {
    const uint32_t nrec = 10000000u, ncloud = 7500000u, nscrub = 32u << 20;      // 160 MB, 120 MB, 512 MB
    const uint32_t per_slab = (nrec + kSlabs - 1) / kSlabs;
    const double rec_bytes = 16.0 * nrec;
    f4 *A, *B, *C, *D, *S, *sink;
    CK(hipMalloc(&A, 16ull * nrec)); CK(hipMalloc(&B, 16ull * nrec)); CK(hipMalloc(&D, 16ull * nrec));
    CK(hipMalloc(&C, 16ull * ncloud)); CK(hipMalloc(&S, 16ull * nscrub)); CK(hipMalloc(&sink, 64));
    k_write<<<blocks(nrec), kT>>>(A, nrec); k_write<<<blocks(nrec), kT>>>(B, nrec); k_write<<<blocks(nrec), kT>>>(D, nrec);
    k_write<<<blocks(ncloud), kT>>>(C, ncloud); k_write<<<blocks(nscrub), kT>>>(S, nscrub);
    CK(hipDeviceSynchronize());
    Timer t;
    auto scrub = [&] { k_read<false><<<blocks(nscrub), kT>>>(S, nscrub, sink); };
    const dim3 gslab(blocks(per_slab), kSlabs);
    printf("{\"bytes_recs\": %.0f, \"bytes_cloud\": %.0f, \"slabs\": %u, \"reps\": %d, \"unit\": \"TB/s, median\"", rec_bytes, 16.0 * ncloud, kSlabs, kReps);

    {   // (a)
        std::vector<double> cold, warm, wr;
        for (int r = 0; r < kReps; ++r) {
            scrub();
            t.start(); k_read<false><<<blocks(nrec), kT>>>(A, nrec, sink); cold.push_back(t.stop_us());
            scrub();
            t.start(); k_write<<<blocks(nrec), kT>>>(A, nrec); wr.push_back(t.stop_us());
            t.start(); k_read<false><<<blocks(nrec), kT>>>(A, nrec, sink); warm.push_back(t.stop_us());
        }
        printf(",\n \"a\": {\"read_cold\": %.2f, \"write\": %.2f, \"read_back\": %.2f, \"read_back_us\": %.1f, \"read_cold_us\": %.1f}",
               tbs(rec_bytes, median(cold)), tbs(rec_bytes, median(wr)), tbs(rec_bytes, median(warm)), median(warm), median(cold));
    }
    {   // (b)
        double rate[2], us[2];
        for (int nt = 0; nt < 2; ++nt) {
            std::vector<double> back;
            for (int r = 0; r < kReps; ++r) {
                scrub();
                k_write<<<blocks(nrec), kT>>>(A, nrec);
                if (nt) { k_read<true><<<blocks(ncloud), kT>>>(C, ncloud, sink); k_read<true><<<blocks(nrec), kT>>>(D, nrec, sink); }
                else { k_read<false><<<blocks(ncloud), kT>>>(C, ncloud, sink); k_read<false><<<blocks(nrec), kT>>>(D, nrec, sink); }
                t.start(); k_read<false><<<blocks(nrec), kT>>>(A, nrec, sink); back.push_back(t.stop_us());
            }
            us[nt] = median(back); rate[nt] = tbs(rec_bytes, us[nt]);
        }
        printf(",\n \"b\": {\"read_back_behind_plain_reads\": %.2f, \"read_back_behind_nt_reads\": %.2f, \"plain_us\": %.1f, \"nt_us\": %.1f}", rate[0], rate[1], us[0], us[1]);
    }
    {   // (c)
        printf(",\n \"c\": {");
        for (int nt = 0; nt < 2; ++nt) for (int rev = 0; rev < 2; ++rev) {
            std::vector<double> prod, cons;
            for (int r = 0; r < kReps; ++r) {
                scrub();
                k_write<<<blocks(nrec), kT>>>(A, nrec);
                t.start();
                if (nt) k_slab_copy<true><<<gslab, kT>>>(A, B, nrec, per_slab); else k_slab_copy<false><<<gslab, kT>>>(A, B, nrec, per_slab);
                prod.push_back(t.stop_us());
                t.start(); k_slab_read<false><<<gslab, kT>>>(B, nrec, per_slab, (uint32_t)rev, sink); cons.push_back(t.stop_us());
            }
            printf("%s\"producer_%s_consumer_%s\": {\"producer_us\": %.1f, \"consumer\": %.2f, \"consumer_us\": %.1f}", (nt | rev) ? ", " : "",
                   nt ? "nt" : "plain", rev ? "descending" : "ascending", median(prod), tbs(rec_bytes, median(cons)), median(cons));
        }
        printf("}");
    }
    {   // (p)
        printf(",\n \"p\": {");
        for (int nt = 0; nt < 2; ++nt) for (int rev = 0; rev < 2; ++rev) {
            std::vector<double> l1, l2, cons;
            for (int r = 0; r < kReps; ++r) {
                scrub();
                t.start();
                if (nt) k_copy<true><<<blocks(nrec), kT>>>(C, ncloud, A, nrec); else k_copy<false><<<blocks(nrec), kT>>>(C, ncloud, A, nrec);
                l1.push_back(t.stop_us());
                t.start();
                if (nt) k_slab_copy<true><<<gslab, kT>>>(A, B, nrec, per_slab); else k_slab_copy<false><<<gslab, kT>>>(A, B, nrec, per_slab);
                l2.push_back(t.stop_us());
                t.start();
                if (nt) k_slab_read<true><<<gslab, kT>>>(B, nrec, per_slab, (uint32_t)rev, sink); else k_slab_read<false><<<gslab, kT>>>(B, nrec, per_slab, (uint32_t)rev, sink);
                cons.push_back(t.stop_us());
            }
            printf("%s\"loads_%s_consumer_%s\": {\"level1_us\": %.1f, \"level2_us\": %.1f, \"consumer_us\": %.1f, \"consumer\": %.2f}", (nt | rev) ? ", " : "",
                   nt ? "nt" : "plain", rev ? "descending" : "ascending", median(l1), median(l2), median(cons), tbs(rec_bytes, median(cons)));
        }
        printf("}");
    }
    printf("}\n");
    CK(hipDeviceSynchronize());
    CK(hipFree(A)); CK(hipFree(B)); CK(hipFree(C)); CK(hipFree(D)); CK(hipFree(S)); CK(hipFree(sink));
    return 0;
}
