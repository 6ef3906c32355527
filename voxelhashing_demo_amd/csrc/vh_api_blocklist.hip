// vh_api_blocklist.hip -- host side of the ordered block list (kernels: vh_blocklist.hip): its scratch and the
// only place that knows the scratch's layout, the list's launches, the two-level scan.  Shared by vh_extract_mesh,
// vh_extract_mesh_indexed, vh_components / vh_remove_components and vh_stream_out.
// Included by vh_api.hip ahead of vh_api_mesh.hip (same translation unit: shares fail(), VH_HIP, grid_for()).

// what the model-reading kernels take: the context's pointers, with the voxels of a view table where they live, in the records
static DevPtrs model_ptrs(const vh_context *c)
{
    DevPtrs dp = c->dp;
    if (c->viewBlocks) dp.blocks = const_cast<Voxel *>(c->viewBlocks);
    return dp;
}

// the blocks a list can hold: a table holds at most numVoxelBlocks blocks, a view table one per imported record
static size_t block_list_capacity(const vh_context *c)
{
    return std::max<size_t>(1, std::min<size_t>(c->numEntries, c->viewBlocks ? (size_t)c->viewCount : (size_t)c->params.numVoxelBlocks));
}

// entries of a map indexed by a block's ptr >> 9 (unique per block: heap blocks lie 512 voxels apart, view records 514)
static size_t ptr_map_size(const vh_context *c)
{
    return c->viewBlocks ? (((size_t)c->viewCount * 514 + 2) >> 9) + 1 : (size_t)c->params.numVoxelBlocks;
}

// no region: every block
static BlockBox block_box(const vh_mesh_region *region)
{
    BlockBox box;
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = region ? region->block_lo[a] : INT32_MIN;
        box.hi[a] = region ? region->block_hi[a] : INT32_MAX;
    }
    return box;
}

static size_t scan_tiles(size_t n) { return (n + kScanTile - 1) / kScanTile; }

// The list's scratch as the calls name it.  meshItems: the list.  meshCounts: the slice counts, then one count per listed block
// for the caller's round.  meshTotals: the slice scan's tile totals, the block scan's, then two result words, [0] the list's
// length (a caller with result words of its own points `result` at them before list_blocks).
struct BlockListScratch {
    int4 *items = nullptr;
    uint32_t listCapacity = 0;             // blocks `items` has room for: at least block_list_capacity(c)
    size_t slices = 0;                     // waves of the list walk
    uint32_t *sliceCount = nullptr, *blockCount = nullptr;
    unsigned long long *sliceTiles = nullptr, *blockTiles = nullptr, *result = nullptr;
};

// Allocated at the first call and kept (grown when a view context imports more records).  All or nothing: a failed allocation
// leaves the context as it was.
static int block_list_reserve(vh_context *c, BlockListScratch &sc)
{
    const size_t slices = ((size_t)c->ownedBuckets + kListSliceBuckets - 1) / kListSliceBuckets, blocks = block_list_capacity(c);
    const size_t counts = slices + blocks, totals = scan_tiles(slices) + scan_tiles(blocks) + 2;
    if (c->meshItems.size() < blocks || c->meshCounts.size() < counts || c->meshTotals.size() < totals) {
        VH_HIP(hipStreamSynchronize(c->stream));           // (before an older, smaller set is freed)
        DevBuf<int4> items;
        DevBuf<uint32_t> cnt;
        DevBuf<unsigned long long> tot;
        int rc;
        if ((rc = items.alloc(blocks, "mesh block list")) || (rc = cnt.alloc(counts, "mesh counts")) ||
            (rc = tot.alloc(totals, "mesh scan totals")))
            return rc;
        c->meshItems = std::move(items);
        c->meshCounts = std::move(cnt);
        c->meshTotals = std::move(tot);
    }
    const size_t listed = c->meshItems.size();             // (of one allocation with the other two: they agree on it)
    sc.items = c->meshItems;
    sc.listCapacity = (uint32_t)listed;
    sc.slices = slices;
    sc.sliceCount = c->meshCounts;
    sc.blockCount = sc.sliceCount + slices;
    sc.sliceTiles = c->meshTotals;
    sc.blockTiles = sc.sliceTiles + scan_tiles(slices);
    sc.result = sc.blockTiles + scan_tiles(listed);
    return VH_OK;
}

// counts[0 .. n) becomes its exclusive scan (tiles[i / kScanTile] + counts[i]: scanned_at), *totalOut the sum, at most `cap`.
// n = *nPtr, a length only the device knows, of which nHost is the host's bound; without nPtr, n = nHost.
static void scan_counts(hipStream_t s, uint32_t *counts, const unsigned long long *nPtr, size_t nHost, unsigned long long *tiles,
                        unsigned long long cap, unsigned long long *totalOut)
{
    hipLaunchKernelGGL(block_scan_tiles_kernel, dim3((unsigned)grid_for(nHost, kScanTile)), dim3(256), 0, s, counts, nPtr,
                       (uint32_t)nHost, tiles);
    hipLaunchKernelGGL(block_scan_totals_kernel, dim3(1), dim3(256), 0, s, tiles, nPtr, (uint32_t)nHost, cap, totalOut);
}

// The entries `pred` selects as sc.items, in ascending entry index; sc.result[0] = their number (at most sc.listCapacity).
// write = false: the number alone.  Reserves the scratch unless the caller has (block_list_reserve); launches only: the
// read-back, the synchronisation and check_spin_timeouts are the caller's.
template <class Pred>
static int list_blocks(vh_context *c, const FrameParams &fp, const DevPtrs &dp, const Pred &pred, bool write, BlockListScratch &sc)
{
    if (!sc.items) { const int rc = block_list_reserve(c, sc); if (rc != VH_OK) return rc; }
    hipStream_t s = c->stream;
    const unsigned grid = (unsigned)grid_for(sc.slices, 4);
    const unsigned long long *tileBase = sc.sliceTiles;
    hipLaunchKernelGGL((block_list_kernel<false, Pred>), dim3(grid), dim3(256), 0, s, fp, dp, pred, c->ownedBuckets,
                       (uint32_t)sc.slices, sc.sliceCount, tileBase, sc.items, sc.listCapacity);
    scan_counts(s, sc.sliceCount, nullptr, sc.slices, sc.sliceTiles, sc.listCapacity, sc.result);
    if (write)
        hipLaunchKernelGGL((block_list_kernel<true, Pred>), dim3(grid), dim3(256), 0, s, fp, dp, pred, c->ownedBuckets,
                           (uint32_t)sc.slices, sc.sliceCount, tileBase, sc.items, sc.listCapacity);
    return VH_OK;
}
