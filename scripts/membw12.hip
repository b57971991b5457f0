// membw12.hip -- does a dictionary-string decode in the linear-fill shape keep
// the fill's write rate?
// (Round 7.  A DICT VARCHAR column is > 98 % stores: 16 B string_t out per
// 1-3 bits in.  The decode writes it as ~4,096 concurrent 1 MiB streams, which
// membw8 measured at 5.3-6.75 TB/s depending on the allocation, while a fill in
// dispatch order, one 4 KiB block per 256-thread workgroup, ran 6.82-6.94 TB/s
// on every allocation.)
//
// One 16 B x N output buffer (c4's shape, N = 2^29 rows = 8 GiB) per trial,
// every trial a new allocation kept until the end, and on it:
//   (a) chunks   1 MiB chunks front to back, 1-wave persistent blocks, 16 per
//                CU, wave w takes chunks w, w + NW, ... (membw8's lpt arm: all
//                chunks are the same size here)
//   (b) fill     one 4 KiB block per 256-thread workgroup, non-persistent
//   (c) wg4/8/16 fill order, but every workgroup first makes the dependent
//                loads of the decode: a 32 B descriptor per 1024-value vector
//                (scalar), then its share of the vector's packed codes (W = 2:
//                256 B per vector), then a 16 B table entry per lane from an
//                8-entry table, and only then stores 4, 8 or 16 KiB (1, 2 or 4
//                back-to-back 4 KiB stores)
// argv: trials (default 8)
//   hipcc -O3 --offload-arch=gfx950 scripts/membw12.hip -o scripts/membw12
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

#define CK(x)                                                                          \
    do {                                                                               \
        hipError_t e = (x);                                                            \
        if (e != hipSuccess) {                                                         \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e));                     \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

struct Desc {  // 32 B per vector
    const uint32_t *packed;
    const v4u *tab;
    v4u *out;
    uint32_t base, info;  // info = nvals | W << 11
};

__global__ __launch_bounds__(64) void k_chunks(v4u *__restrict__ out, uint32_t nchunks) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        v4u *o = out + (size_t)c * 65536;
        const v4u x = {lane, c, 7u, 9u};
        for (uint32_t i = 0; i < 1024; ++i) o[i * 64 + lane] = x + i;
    }
}

__global__ __launch_bounds__(256) void k_fill(v4u *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    out[i] = v4u{(uint32_t)i, 1u, 2u, 3u};
}

typedef const __attribute__((address_space(1))) uint32_t gu32;
typedef const __attribute__((address_space(1))) v4u gv4;
typedef __attribute__((address_space(1))) v4u ov4;

// K 4 KiB stores per workgroup (K <= 4: 4 / K workgroups per vector, else K / 4
// vectors per workgroup).  Pointers out of the descriptor are cast to the
// global address space (else hipcc emits flat_* accesses).  LDS: the table is
// staged into LDS by the workgroup, its load issued beside the packed loads
// (both wait for the descriptor only), so the chain is two global round trips
// (1: one copy per workgroup behind a barrier, "l" arms; 2: one copy per wave
// and no barrier, "w" arms).
template <int K, int LDS>
__global__ __launch_bounds__(256) void k_wg(const Desc *__restrict__ descs) {
    constexpr int NV = (K + 3) / 4;
    __shared__ v4u stab_all[(LDS == 2 ? 4 : 1) * NV * 8];
    const uint32_t t = threadIdx.x, q0 = blockIdx.x * K;
    Desc d[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) d[v] = descs[q0 / 4 + v];
    v4u *stab = stab_all + (LDS == 2 ? (t >> 6) * NV * 8 : 0);  // LDS == 2: a copy per wave, no barrier
    const uint32_t ts = LDS == 2 ? (t & 63) : t;
    if (LDS && ts < NV * 8) stab[ts] = ((gv4 *)d[0].tab)[ts & 7];  // (one table here; per vector in a decode)
    uint32_t code[K];
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const Desc &x = d[r / 4];
        const uint32_t W = (x.info >> 11) & 63, mask = W >= 32 ? 0xFFFFFFFFu : (1u << W) - 1u;
        const uint32_t p = ((q0 + r) & 3) * 256 + t, bit = (p >> 5) * W, k = bit >> 5;
        gu32 *pk = (gu32 *)x.packed;
        const uint32_t lo = pk[k * 32 + (p & 31)], hi = pk[min(k + 1, W - 1) * 32 + (p & 31)];
        code[r] = (__builtin_amdgcn_alignbit(hi, lo, bit & 31) & mask) + x.base;
    }
    v4u e[K];
    if (LDS == 1) __syncthreads();
#pragma unroll
    for (int r = 0; r < K; ++r) e[r] = LDS ? stab[(r / 4) * 8 + (code[r] & 7)] : ((gv4 *)d[r / 4].tab)[code[r] & 7];
#pragma unroll
    for (int r = 0; r < K; ++r) {
        const Desc &x = d[r / 4];
        const uint32_t p = ((q0 + r) & 3) * 256 + t;
        if (p < (x.info & 2047)) ((ov4 *)x.out)[p] = e[r];
    }
}

int main(int argc, char **argv) {
    const int trials = argc > 1 ? std::max(1, atoi(argv[1])) : 8;
    const uint64_t rows = 1ull << 29, bytes = rows * 16;
    const uint32_t nvec = (uint32_t)(rows / 1024), W = 2;
    int cus = 256;
    CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    const int grid = cus * 16;
    // packed codes (W word-rows of 128 B per vector) and the table, shared by the trials
    uint32_t *packed;
    v4u *tab;
    Desc *descs;
    CK(hipMalloc(&packed, (size_t)nvec * W * 128));
    CK(hipMalloc(&tab, 8 * 16));
    CK(hipMalloc(&descs, (size_t)nvec * sizeof(Desc)));
    {
        std::vector<uint32_t> h((size_t)nvec * W * 32);
        uint32_t x = 12345;
        for (auto &w : h) w = (x = x * 1664525u + 1013904223u);
        CK(hipMemcpy(packed, h.data(), h.size() * 4, hipMemcpyHostToDevice));
        v4u ht[8];
        for (uint32_t i = 0; i < 8; ++i) ht[i] = v4u{i, i + 1, i + 2, i + 3};
        CK(hipMemcpy(tab, ht, sizeof(ht), hipMemcpyHostToDevice));
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    auto timeit = [&](auto launch) {
        launch();
        CK(hipDeviceSynchronize());
        float sum = 0;
        for (int r = 0; r < 6; ++r) {
            CK(hipEventRecord(e0));
            launch();
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            sum += ms;
        }
        return sum / 6;
    };
    std::vector<char *> bufs;
    constexpr int NA = 14;
    std::vector<float> col[NA];
    printf("rows %llu, %d CUs, GB/s written (mean of 6 launches)\n", (unsigned long long)rows, cus);
    const char *names[NA] = {"chunks", "fill", "wg4", "wg8", "wg16", "wg32", "wg64", "wg4l", "wg8l", "wg16l", "wg32l", "wg64l", "wg16w", "wg32w"};
    printf("%-16s", "allocation");
    for (int a = 0; a < NA; ++a) printf(" %6s", names[a]);
    printf("\n");
    for (int tr = 0; tr < trials; ++tr) {
        char *buf;
        CK(hipMalloc(&buf, bytes));
        bufs.push_back(buf);
        std::vector<Desc> h(nvec);
        for (uint32_t v = 0; v < nvec; ++v)
            h[v] = Desc{packed + (size_t)v * W * 32, tab, (v4u *)buf + (size_t)v * 1024, 0u, 1024u | W << 11};
        CK(hipMemcpy(descs, h.data(), h.size() * sizeof(Desc), hipMemcpyHostToDevice));
        const float ms[NA] = {
            timeit([&] { k_chunks<<<grid, 64>>>((v4u *)buf, (uint32_t)(bytes >> 20)); }),
            timeit([&] { k_fill<<<(unsigned)(bytes / 4096), 256>>>((v4u *)buf); }),
            timeit([&] { k_wg<1, 0><<<nvec * 4, 256>>>(descs); }),
            timeit([&] { k_wg<2, 0><<<nvec * 2, 256>>>(descs); }),
            timeit([&] { k_wg<4, 0><<<nvec, 256>>>(descs); }),
            timeit([&] { k_wg<8, 0><<<nvec / 2, 256>>>(descs); }),
            timeit([&] { k_wg<16, 0><<<nvec / 4, 256>>>(descs); }),
            timeit([&] { k_wg<1, 1><<<nvec * 4, 256>>>(descs); }),
            timeit([&] { k_wg<2, 1><<<nvec * 2, 256>>>(descs); }),
            timeit([&] { k_wg<4, 1><<<nvec, 256>>>(descs); }),
            timeit([&] { k_wg<8, 1><<<nvec / 2, 256>>>(descs); }),
            timeit([&] { k_wg<16, 1><<<nvec / 4, 256>>>(descs); }),
            timeit([&] { k_wg<4, 2><<<nvec, 256>>>(descs); }),
            timeit([&] { k_wg<8, 2><<<nvec / 2, 256>>>(descs); }),
        };
        printf("%-16p", (void *)buf);
        for (int a = 0; a < NA; ++a) {
            const float g = bytes / ms[a] / 1e6f;
            col[a].push_back(g);
            printf(" %6.0f", g);
        }
        printf("\n");
        fflush(stdout);
    }
    printf("%-16s", "median");
    for (int a = 0; a < NA; ++a) {
        std::sort(col[a].begin(), col[a].end());
        const size_t n = col[a].size();
        printf(" %6.0f", n % 2 ? col[a][n / 2] : 0.5f * (col[a][n / 2 - 1] + col[a][n / 2]));
    }
    printf("\n%-16s", "min");
    for (int a = 0; a < NA; ++a) printf(" %6.0f", col[a].front());
    printf("\n%-16s", "max");
    for (int a = 0; a < NA; ++a) printf(" %6.0f", col[a].back());
    printf("\n");
    for (char *b : bufs) CK(hipFree(b));
    return 0;
}
