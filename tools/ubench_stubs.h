// ubench_stubs.h — the three pieces of s3d_runtime.hip that the stand-alone tools need without linking the library: options read
// from the environment (S3D_<NAME> at every query, no range check), the rider switch (S3D_RIDERS) and the compute-unit count of the current device.
// Included after s3d_common.h.
#pragma once
#include <cstdlib>
#include <cstring>
#include <string>

namespace s3d {
int opt(Opt o) {
    const char* e = getenv((std::string("S3D_") + kOptNames[o]).c_str());
    if (!e) return kOptUnset;
    return o == OPT_CONV_IMPL ? (strcmp(e, "naive") == 0 ? 1 : 0) : atoi(e);
}
bool riders_enabled() {
    const char* e = getenv("S3D_RIDERS");
    return !(e && strcmp(e, "0") == 0);
}
int device_cus() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
        return 256;
    return n;
}
}  // namespace s3d
