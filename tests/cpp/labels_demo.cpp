// Labels through the C++ SDF_Hashtable facade: a small model fused from three 64x48 depth frames (uint16 sensor images; 2^11
// buckets, 4 cm voxels, 512 blocks, PINHOLE semantics), labelled with integrateLabels() from their registered label images, then
// sampleLabels() at the given points, labelCounts(), removeLabel() and labelCounts() again.
//   labels_demo <frames.bin: 3 * 64*48 uint16> <labels.bin: 3 * 64*48 uint16> <poses.bin: 3 * 16 floats> <kinv.bin: 9 floats>
//               <points.bin: n*3 floats> <band> <vote max> <min votes> <bins> <label to remove>
// prints "points=<n> labelled=<k>", one line of n words in hex, "counts <bins numbers>", then per allocated block
// "key x y z <checksum>" (the sum over the block's 512 label words of word[i] * (2 i + 1), modulo 2^64), then
// "removed blocks=<b> voxels=<v> freed=<f>" and "counts <bins numbers>" after the removal
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "SDF_Hashtable.h"

static bool read_all(const char *path, void *dst, size_t bytes)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    const bool ok = std::fread(dst, 1, bytes, f) == bytes;
    std::fclose(f);
    return ok;
}

static void print_counts(const std::vector<uint32_t> &counts)
{
    std::printf("counts");
    for (uint32_t c : counts) std::printf(" %u", c);
    std::printf("\n");
}

int main(int argc, char **argv)
{
    if (argc < 11) return 2;
    const int W = 64, H = 48;
    const size_t n = (size_t)W * H;
    std::vector<uint16_t> images(3 * n), labels(3 * n);
    float poses[3][16], kInv[9];
    if (!read_all(argv[1], images.data(), images.size() * sizeof(uint16_t)) ||
        !read_all(argv[2], labels.data(), labels.size() * sizeof(uint16_t)) || !read_all(argv[3], poses, sizeof poses) ||
        !read_all(argv[4], kInv, sizeof kInv))
        return 3;
    std::vector<float> points;
    FILE *f = std::fopen(argv[5], "rb");
    if (!f) return 3;
    float xyz[3];
    while (std::fread(xyz, sizeof(float), 3, f) == 3) points.insert(points.end(), xyz, xyz + 3);
    std::fclose(f);
    const float band = (float)std::atof(argv[6]);
    const int voteMax = std::atoi(argv[7]), minVotes = std::atoi(argv[8]), bins = std::atoi(argv[9]), doomed = std::atoi(argv[10]);
    uint16_t *d_images = nullptr, *d_labels = nullptr;
    if (hipMalloc((void **)&d_images, images.size() * sizeof(uint16_t)) != hipSuccess ||
        hipMalloc((void **)&d_labels, labels.size() * sizeof(uint16_t)) != hipSuccess)
        return 4;
    (void)hipMemcpy(d_images, images.data(), images.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
    (void)hipMemcpy(d_labels, labels.data(), labels.size() * sizeof(uint16_t), hipMemcpyHostToDevice);

    HashTableParams p;
    vh_default_params(&p);
    p.numBuckets = 1u << 11;
    p.voxelSize = 0.04f;
    p.numVoxelBlocks = 512;
    SDF_Hashtable table(p, W, H, VH_SEM_PINHOLE);
    for (int i = 0; i < 3; ++i) table.integrate(float4x4(poses[i]), d_images + i * n, kInv);
    for (int i = 0; i < 3; ++i) table.integrateLabels(float4x4(poses[i]), d_images + i * n, kInv, d_labels + i * n, band, voteMax);

    std::vector<uint32_t> words, counts;
    table.sampleLabels(points, words, minVotes);
    if (words.size() != points.size() / 3) return 6;
    size_t have = 0;
    for (uint32_t w : words) have += w != 0u;
    std::printf("points=%zu labelled=%zu\n", points.size() / 3, have);
    for (uint32_t w : words) std::printf("%08x ", w);
    std::printf("\n");
    table.labelCounts(bins, counts, nullptr, minVotes);
    print_counts(counts);

    std::vector<VoxelEntry> entries((size_t)p.numBuckets * p.bucketSize);
    std::vector<uint32_t> volume((size_t)p.numVoxelBlocks * 512);
    if (!vh_has_labels(table.context()) ||
        vh_download(table.context(), VH_BUF_HASH_TABLE, entries.data(), entries.size() * sizeof(VoxelEntry)) != VH_OK ||
        vh_download_labels(table.context(), 0, volume.data(), volume.size()) != VH_OK)
        return 5;
    for (const VoxelEntry &e : entries) {
        if (e.ptr == VH_FREE_BLOCK) continue;
        unsigned long long sum = 0;
        for (unsigned i = 0; i < 512; ++i) sum += (unsigned long long)volume[(size_t)e.ptr + i] * (2ull * i + 1ull);
        std::printf("key %d %d %d %llu\n", e.pos[0], e.pos[1], e.pos[2], sum);
    }
    const vh_label_stats st = table.removeLabel(doomed, minVotes);
    std::printf("removed blocks=%llu voxels=%llu freed=%llu\n", (unsigned long long)st.blocks, (unsigned long long)st.removed_voxels,
                (unsigned long long)st.freed_blocks);
    table.labelCounts(bins, counts, nullptr, minVotes);
    print_counts(counts);
    (void)hipFree(d_images);
    (void)hipFree(d_labels);
    return 0;
}
