// vh_esdf.hip -- the Euclidean distance to the surface on the voxel lattice: vh_esdf_lattice (the rule is in
// include/voxelhash.h, "the model as a distance field", and tests/esdf_ref.py states it by definition).
// Part of libvoxelhash_hip.so (gfx950); included by vh_kernels.hip after vh_sample.hip (sample_judge, sample_index; lookup_block
// comes from vh_raycast.hip).
//
// An exact, capped, signed squared distance transform in integers, separable over the axes.  With G = the box grown by R:
//   esdf_classify_kernel   one workgroup pass per 8^3 brick of G (sample_lattice_kernel's pass): one lookup, a wave's ballot
//                          over 64 voxels is eight row bytes of a bit plane.  Two planes (inside, outside), packed along x.
//   esdf_row_kernel        x: per voxel the nearest set bit within +-R of its row, in both planes, by count-leading /
//                          count-trailing zeros over the 64-bit words a wave's voxels can reach (wave-uniform: scalar loads):
//                          uint16 d^2, 0xFFFF = none.
//   esdf_axis_kernel       y, then z: out[t] = min over o of in[t + o] + o^2, lanes along the contiguous axis (every access a
//                          whole line).  A lane keeps eight consecutive outputs of its column in registers and walks the
//                          8 + 2R inputs they depend on once, so a loaded value serves eight outputs; the four waves of a
//                          workgroup take neighbouring runs of the same columns and meet in the vector L1.  Both fields (to the
//                          nearest inside voxel P, to the nearest outside voxel N) go through together.  The z pass ends with
//                          the selection by the voxel's own class and writes the int32 and / or float outputs.
// A partial d^2 above R^2 cannot become a total <= R^2 and is stored as "none"; "none" + o^2 > R^2 drops out by itself.
#pragma once

namespace vh {

constexpr int kEsdfMaxRadius = 255;
constexpr uint32_t kEsdfNone16 = 0xFFFFu;
constexpr int kEsdfUnknownKeep = 0, kEsdfUnknownFree = 1, kEsdfUnknownOccupied = 2;
constexpr int kEsdfRun = 8;                  // outputs a lane keeps in registers along the pass axis
constexpr int kEsdfTileAxis = 4 * kEsdfRun;  // ... and a workgroup of four waves

// The layout of a call: everything in voxels of the grown box, whose x starts at a multiple of 8 (whole brick bytes).
//   planes   [gz][gy][words] 64-bit words, bit (x - gx0) of a row; inside first, then outside
//   rows     after x:  [gz][gy][dx] uint16, P then N
//   cols     after y:  [gz][dy][dx] uint16, P then N
struct EsdfLayout {
    int lo[3], dims[3];
    int radius, unknown;
    int gx0;                                 // x of bit 0 of a plane row: (lo[0] - R) rounded down to 8
    int glo[2];                              // y and z of row 0: lo - R
    unsigned long long gy, gz;               // rows of the grown box
    unsigned long long words;                // 64-bit words of a plane row
    int brick0[3], bricks[3];                // classification: first brick, bricks per axis (x: words * 8)
};

// ---------------------------------------------------------------------------------------------------------------------
// classify
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void esdf_classify_kernel(const FrameParams fp, const DevPtrs dp, const EsdfLayout L,
                                                            unsigned long long numBricks,
                                                            unsigned long long *__restrict__ planeIn,
                                                            unsigned long long *__restrict__ planeOut)
{
    __shared__ int sPtr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = lane & 7, y = lane >> 3;                                 // the wave's 64 voxels: one z slice, x fastest
    uint8_t *const inBytes = reinterpret_cast<uint8_t *>(planeIn);
    uint8_t *const outBytes = reinterpret_cast<uint8_t *>(planeOut);
    const unsigned long long rowBytes = L.words * 8ull;
    const long long xEnd = (long long)L.lo[0] + L.dims[0] + L.radius;       // first x beyond the grown box
    for (unsigned long long b = blockIdx.x; b < numBricks; b += gridDim.x) {
        const unsigned long long row = b / (unsigned long long)L.bricks[0];
        const int ix = (int)(b - row * (unsigned long long)L.bricks[0]);
        const int bx = L.brick0[0] + ix;
        const int by = L.brick0[1] + (int)(row % (unsigned long long)L.bricks[1]);
        const int bz = L.brick0[2] + (int)(row / (unsigned long long)L.bricks[1]);
        __syncthreads();                            // (the pass before has read sPtr)
        // (the bricks that pad a row to whole words lie beyond the grown box: no site of theirs is within R of the box)
        if (threadIdx.x == 0) sPtr = (long long)bx * 8 < xEnd ? lookup_block(fp, dp, bx, by, bz) : VH_FREE_BLOCK;
        __syncthreads();
        const int ptr = sPtr;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int z = wave + 4 * half;
            SampleVoxel v = {__builtin_nanf(""), 0.0f};
            if (ptr != VH_FREE_BLOCK) {
                const Voxel s = dp.blocks[(size_t)ptr + (size_t)sample_index(x, y, z)];
                v = sample_judge(s.sdf, s.weight);
            }
            const bool valid = v.sdf == v.sdf;
            bool inside = valid && v.sdf < 0.0f, outside = valid && !inside;
            if (L.unknown == kEsdfUnknownFree) outside = !inside;
            if (L.unknown == kEsdfUnknownOccupied) inside = !outside;
            const unsigned long long bitsIn = __ballot(inside), bitsOut = __ballot(outside);     // byte y = row (y, z) of the brick
            const long long j = (long long)by * 8 + lane - L.glo[0], k = (long long)bz * 8 + z - L.glo[1];
            if (lane < 8 && j >= 0 && j < (long long)L.gy && k >= 0 && k < (long long)L.gz) {
                const unsigned long long at = ((unsigned long long)k * L.gy + (unsigned long long)j) * rowBytes + (unsigned long long)ix;
                inBytes[at] = (uint8_t)(bitsIn >> (8 * lane));
                outBytes[at] = (uint8_t)(bitsOut >> (8 * lane));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// x
// ---------------------------------------------------------------------------------------------------------------------
// The distance from a voxel to the nearest set bit of one 64-bit word of its row; q = the voxel's position relative to the
// word's bit 0 (below 0 or above 63 when the word lies beside the voxel).  No bit: a distance beyond any radius.
__device__ __forceinline__ int esdf_word_distance(unsigned long long m, int q)
{
    const int qc = min(max(q, 0), 63);
    const unsigned long long above = q > 63 ? 0ull : m & (~0ull << qc);                // bits at or above the voxel
    const unsigned long long below = q < 0 ? 0ull : m & (~0ull >> (63 - qc));          // bits at or below it
    const int up = above ? __builtin_ctzll(above) - q : 1 << 20;
    const int down = below ? q - (63 - __builtin_clzll(below)) : 1 << 20;
    return min(up, down);
}

// One lane per voxel of [gz][gy][dx], x fastest; a workgroup takes 256 consecutive x of one row at a time.  The words within R
// of a wave's 64 voxels are the same for all its lanes (2 + R / 32 of them at most): they are read once per wave, through the
// scalar path, and every lane takes its minimum over them -- no per-lane loop, no per-lane loads.
__global__ __launch_bounds__(256) void esdf_row_kernel(const EsdfLayout L, unsigned long long numTiles, unsigned long long tilesX,
                                                       const unsigned long long *__restrict__ planeIn,
                                                       const unsigned long long *__restrict__ planeOut,
                                                       uint16_t *__restrict__ rowsP, uint16_t *__restrict__ rowsN)
{
    const int xoff = L.lo[0] - L.gx0;              // bit of the box's first voxel
    const int R = L.radius, words = (int)L.words;
    for (unsigned long long t = blockIdx.x; t < numTiles; t += gridDim.x) {
        const unsigned long long row = t / tilesX;
        const unsigned long long i0 = (t - row * tilesX) * 256ull + (threadIdx.x & ~63u);      // the wave's first voxel
        if (i0 >= (unsigned long long)L.dims[0]) continue;                                     // (the whole wave)
        const int p0 = __builtin_amdgcn_readfirstlane((int)i0 + xoff);
        const int first = max(0, (p0 - R) >> 6), last = min(words - 1, (p0 + 63 + R) >> 6);
        const unsigned long long *__restrict__ in = planeIn + row * L.words, *__restrict__ out = planeOut + row * L.words;
        const int p = p0 + (int)(threadIdx.x & 63u);
        int bestP = R + 1, bestN = R + 1;
        for (int w = first; w <= last; ++w) {
            const unsigned long long mIn = in[w], mOut = out[w];           // (wave-uniform: an empty word costs a branch)
            if (mIn) bestP = min(bestP, esdf_word_distance(mIn, p - 64 * w));
            if (mOut) bestN = min(bestN, esdf_word_distance(mOut, p - 64 * w));
        }
        const unsigned long long i = i0 + (threadIdx.x & 63u);
        if (i >= (unsigned long long)L.dims[0]) continue;
        const unsigned long long at = row * (unsigned long long)L.dims[0] + i;
        rowsP[at] = (uint16_t)(bestP <= R ? bestP * bestP : (int)kEsdfNone16);
        rowsN[at] = (uint16_t)(bestN <= R ? bestN * bestN : (int)kEsdfNone16);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// y and z
// ---------------------------------------------------------------------------------------------------------------------
// A min-plus pass along one axis: in [outer][lenOut + 2R][inner] -> out [outer][lenOut][inner], out[t] = min over rows r of
// in[r] + (r - R - t)^2 (rows further than R from t add more than R^2 and drop out with the cap).
struct EsdfAxis {
    unsigned long long inner;                // elements of the contiguous axes (lanes run along them)
    unsigned long long lenOut;               // outputs along the pass axis
    unsigned long long tilesInner, tilesAxis, numTiles;      // 64 inner x kEsdfTileAxis outputs per tile; numTiles includes `outer`
    int radius;
};

struct EsdfSelect {                          // the z pass: selection and the outputs
    const unsigned long long *planeIn, *planeOut;
    int32_t *dist2;
    float *distance;
    float voxelSize;
};

template <bool kSelect>
__global__ __launch_bounds__(256) void esdf_axis_kernel(const EsdfAxis A, const EsdfLayout L, const uint16_t *__restrict__ inP,
                                                        const uint16_t *__restrict__ inN, uint16_t *__restrict__ outP,
                                                        uint16_t *__restrict__ outN, const EsdfSelect S)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int R = A.radius;
    const uint32_t cap = (uint32_t)(R * R);
    const unsigned long long lenIn = A.lenOut + 2ull * (unsigned long long)R;
    for (unsigned long long tile = blockIdx.x; tile < A.numTiles; tile += gridDim.x) {
        const unsigned long long tInner = tile % A.tilesInner, rest = tile / A.tilesInner;
        const unsigned long long tAxis = rest % A.tilesAxis, outer = rest / A.tilesAxis;
        const unsigned long long col = tInner * 64ull + lane;
        const unsigned long long t0 = tAxis * (unsigned long long)kEsdfTileAxis + (unsigned long long)(wave * kEsdfRun);
        if (col >= A.inner || t0 >= A.lenOut) continue;                    // (no barrier in this kernel)
        const int count = A.lenOut - t0 < (unsigned long long)kEsdfRun ? (int)(A.lenOut - t0) : kEsdfRun;
        uint32_t accP[kEsdfRun], accN[kEsdfRun];
#pragma unroll
        for (int u = 0; u < kEsdfRun; ++u) accP[u] = accN[u] = kEsdfNone16;
        // input row t0 + r is at offset r - R from output t0; the last one any of the run's outputs can use is count - 1 + 2R
        const uint16_t *pP = inP + (outer * lenIn + t0) * A.inner + col;
        const uint16_t *pN = inN + (outer * lenIn + t0) * A.inner + col;
        const int rows = count + 2 * R;
        for (int r = 0; r < rows; ++r) {
            const uint32_t vP = pP[(unsigned long long)r * A.inner], vN = pN[(unsigned long long)r * A.inner];
            if (__ballot((vP & vN) != kEsdfNone16) == 0ull) continue;      // a row of "none" for the whole wave changes no minimum
#pragma unroll
            for (int u = 0; u < kEsdfRun; ++u) {
                const int o = r - R - u;
                const uint32_t oo = (uint32_t)(o * o);
                accP[u] = min(accP[u], vP + oo);
                accN[u] = min(accN[u], vN + oo);
            }
        }
        // the z pass: the eight voxels of the run are (i, j, t0 + u) of the box, col = j * dx + i; their class bits sit at the same
        // bit of words one plane slice apart
        unsigned long long word = 0, sliceWords = 0;
        int shift = 0;
        if (kSelect) {
            const unsigned long long j = col / (unsigned long long)L.dims[0], i = col - j * (unsigned long long)L.dims[0];
            const unsigned long long bit = i + (unsigned long long)(L.lo[0] - L.gx0);
            sliceWords = L.gy * L.words;
            word = ((t0 + (unsigned long long)R) * L.gy + j + (unsigned long long)R) * L.words + (bit >> 6);
            shift = (int)(bit & 63);
        }
#pragma unroll
        for (int u = 0; u < kEsdfRun; ++u) {
            if (u >= count) break;
            const uint32_t P = accP[u] <= cap ? accP[u] : kEsdfNone16, N = accN[u] <= cap ? accN[u] : kEsdfNone16;
            const unsigned long long at = (outer * A.lenOut + t0 + (unsigned long long)u) * A.inner + col;
            if (!kSelect) {
                outP[at] = (uint16_t)P;
                outN[at] = (uint16_t)N;
            } else {
                const unsigned long long w = word + (unsigned long long)u * sliceWords;
                const bool inside = (S.planeIn[w] >> shift) & 1ull, outside = (S.planeOut[w] >> shift) & 1ull;
                int32_t d = INT32_MIN;                                         // VH_ESDF_NONE
                if (outside) d = P == kEsdfNone16 ? INT32_MAX : (int32_t)P;
                else if (inside) d = N == kEsdfNone16 ? -INT32_MAX : -(int32_t)N;
                if (S.dist2) S.dist2[at] = d;
                if (S.distance) {
                    float f = __builtin_nanf("");
                    if (outside || inside) {
                        const uint32_t m = outside ? P : N;
                        f = m == kEsdfNone16 ? __builtin_inff() : __builtin_sqrtf((float)m) * S.voxelSize;
                        if (inside) f = -f;
                    }
                    S.distance[at] = f;
                }
            }
        }
    }
}

}  // namespace vh
