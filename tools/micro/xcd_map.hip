// Placement probe: which XCC (XCD) does workgroup b of a 1-D grid run on, and is that the same in every launch?
// The alternating table walk (vh_walk.hip: walk_tile) keeps a tile on "the XCD of blockIdx % 8" from one launch to the
// next; this program says whether that label is stable.  Every grid is launched kLaunches times back to back on one
// stream; lane 0 of every workgroup stores its HW_REG_XCC_ID.  Reported per grid size:
//   (a) do workgroups b and b + 8 share an XCC inside a launch (every class b % 8 on exactly one XCC)?
//   (b) is the map class -> XCC the same in every launch of the series, and in a series of mixed grids?
//   hipcc --offload-arch=gfx950 -O2 -o xcd_map xcd_map.hip && ./xcd_map
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

constexpr int kLaunches = 8;

__global__ __launch_bounds__(256) void record_xcc(unsigned char *out, const float *__restrict__ work, float *sink)
{
    if (threadIdx.x == 0) {
        unsigned id;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
        out[blockIdx.x] = (unsigned char)(id & 15u);
    }
    // a few hundred nanoseconds of work per workgroup, so that a grid of thousands is not placed on an empty chip throughout
    float acc = 0.0f;
    for (int j = 0; j < 4; ++j) acc += work[(size_t)blockIdx.x * 1024 + j * 256 + threadIdx.x];
    if (acc == 12345.678f) *sink = acc;
}

struct Series { std::vector<std::vector<unsigned char>> launches; };

// class -> XCC of one launch: -1 where a class is spread over several XCCs
static void class_map(const std::vector<unsigned char> &x, int map[8], int &mixed)
{
    mixed = 0;
    for (int q = 0; q < 8; ++q) map[q] = -2;
    for (size_t b = 0; b < x.size(); ++b) {
        int &m = map[b & 7];
        if (m == -2) m = x[b];
        else if (m != (int)x[b]) { if (m != -1) m = -1; ++mixed; }
    }
}

int main()
{
    const int grids[] = {8, 64, 1024, 5760, 6584, 6592, 1023, 1027, 6585, 6587};
    int maxGrid = 0;
    for (int g : grids) maxGrid = g > maxGrid ? g : maxGrid;
    unsigned char *dOut;
    float *dWork, *dSink;
    CK(hipMalloc(&dOut, (size_t)maxGrid * kLaunches * 2));
    CK(hipMalloc(&dWork, (size_t)maxGrid * 1024 * sizeof(float)));
    CK(hipMemset(dWork, 0, (size_t)maxGrid * 1024 * sizeof(float)));
    CK(hipMalloc(&dSink, sizeof(float)));
    hipStream_t s;
    CK(hipStreamCreate(&s));
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    printf("device: %s, %d CUs\n", prop.gcnArchName, prop.multiProcessorCount);
    printf("grid   mult8  (a) b,b+8 share an XCC in every launch   (b) class->XCC equal in all %d launches   map of launch 0 (class 0..7)\n", kLaunches);
    for (int g : grids) {
        for (int l = 0; l < kLaunches; ++l)
            hipLaunchKernelGGL(record_xcc, dim3(g), dim3(256), 0, s, dOut + (size_t)l * g, dWork, dSink);
        CK(hipStreamSynchronize(s));
        std::vector<unsigned char> h((size_t)g * kLaunches);
        CK(hipMemcpy(h.data(), dOut, h.size(), hipMemcpyDeviceToHost));
        bool a = true, b = true;
        int first[8], mixedTotal = 0;
        for (int l = 0; l < kLaunches; ++l) {
            std::vector<unsigned char> x(h.begin() + (size_t)l * g, h.begin() + (size_t)(l + 1) * g);
            int map[8], mixed;
            class_map(x, map, mixed);
            mixedTotal += mixed;
            if (mixed) a = false;
            if (l == 0) for (int q = 0; q < 8; ++q) first[q] = map[q];
            else for (int q = 0; q < 8; ++q) if (map[q] != first[q]) b = false;
        }
        printf("%-6d %-6s %-48s %-42s", g, g % 8 == 0 ? "yes" : "no", a ? "yes" : "NO", b ? "yes" : "NO");
        for (int q = 0; q < 8 && q < g; ++q) printf(" %d", first[q]);
        if (!a) printf("   (%d workgroups off their class's XCC)", mixedTotal);
        printf("\n");
        if (!b && g <= 6592) {
            printf("         class 0's XCC per launch:");
            for (int l = 0; l < kLaunches; ++l) printf(" %d", (int)h[(size_t)l * g]);
            printf("\n");
        }
    }
    // a mixed series, as a batch of frames behind another kernel would be: does a grid that is no multiple of 8 shift
    // the map of the multiple-of-8 launch behind it?
    {
        const int seq[] = {6592, 6592, 1027, 6592, 6585, 6592, 13, 6592};
        size_t off = 0;
        std::vector<size_t> offs;
        for (int g : seq) { offs.push_back(off); hipLaunchKernelGGL(record_xcc, dim3(g), dim3(256), 0, s, dOut + off, dWork, dSink); off += g; }
        CK(hipStreamSynchronize(s));
        std::vector<unsigned char> h(off);
        CK(hipMemcpy(h.data(), dOut, off, hipMemcpyDeviceToHost));
        printf("mixed series (grid: XCC of workgroups 0..7):\n");
        for (size_t i = 0; i < offs.size(); ++i) {
            printf("  %-6d", seq[i]);
            for (int q = 0; q < 8 && q < seq[i]; ++q) printf(" %d", (int)h[offs[i] + q]);
            printf("\n");
        }
    }
    CK(hipFree(dOut)); CK(hipFree(dWork)); CK(hipFree(dSink));
    return 0;
}
