// Tracking against the model through the C++ facade: two frames of one vertex map at the identity pose (as sample_demo.cpp),
// then CameraTracking::AlignToModel of the same vertex map from the given start pose.
//   sdf_track_demo <verts.bin: 640*480 float4> <start.bin: 16 floats> <out.bin>
// writes the 16 floats of the aligned pose; prints "steps=<k> error=<summed residual>"
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "CameraTracking.h"

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const size_t n = 640 * 480;
    std::vector<vh_float4> h_verts(n);
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(h_verts.data(), sizeof(vh_float4), n, f) != n) return 3;
    std::fclose(f);
    float4x4 pose;
    f = std::fopen(argv[2], "rb");
    if (!f || std::fread(pose.entries, sizeof(float), 16, f) != 16) return 3;
    std::fclose(f);
    vh_float4 *d_verts = nullptr;
    if (hipMalloc((void **)&d_verts, n * sizeof(vh_float4)) != hipSuccess) return 4;
    (void)hipMemcpy(d_verts, h_verts.data(), n * sizeof(vh_float4), hipMemcpyHostToDevice);

    SDF_Hashtable table;                         // common.h defaults, REFERENCE semantics
    float4x4 identity;
    identity.setIdentity();
    table.integrate(identity, d_verts, (const vh_float4 *)nullptr);
    table.integrate(identity, d_verts, (const vh_float4 *)nullptr);
    CameraTracking tracker(640, 480);
    const int steps = tracker.AlignToModel(table, d_verts, pose);
    FILE *out = std::fopen(argv[3], "wb");
    if (!out) return 5;
    std::fwrite(pose.entries, sizeof(float), 16, out);
    std::fclose(out);
    std::printf("steps=%d error=%.9g\n", steps, (double)tracker.lastError());
    (void)hipFree(d_verts);
    return 0;
}
