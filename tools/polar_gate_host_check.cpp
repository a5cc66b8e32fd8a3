// polar_gate_host_check.cpp -- stand-alone check of the host side of the polar gates under the sanitizers:
//     g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread
//         tools/polar_gate_host_check.cpp aprilsam_amd/csrc/{capi,host_objects,ordering,symbolic,refmodel,graph_io,errors}.cpp
//         tests/support/solver_nodevice.cpp -o build/polar_gate_host_check && build/polar_gate_host_check
// Calls aprilsam_amd_debug_polar_gate -- the function host and kernels share -- for every kind with a 6 x 6 block on the heap and exactly
// as many z / W entries as the kind may read (a read past them is the sanitizer's finding), its refusals, and the argument checks
// aprilsam_amd_gate_polar / aprilsam_amd_associate_polar make before they ask for a device (polar_gate_args; the entry points themselves
// live in the HIP translation unit).  Exits 0 and prints "ok".  No device, nothing loaded into an interpreter.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../aprilsam_amd/csrc/polar.h"
#include "../include/aprilsam_amd.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "polar_gate_host_check: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main() {
    const double pa[3] = { 1.0, 2.0, 0.5 }, pb[3] = { 2.5, 3.0, -0.7 };
    std::vector<double> zero(36, 0.0), eye(36, 0.0);
    for (int i = 0; i < 6; i++) eye[7 * i] = 1e-2;
    for (int kind = APRILSAM_AMD_POLAR_RANGE; kind <= APRILSAM_AMD_POLAR_RANGE_BEARING; kind++) {
        const int m = kind == APRILSAM_AMD_POLAR_RANGE_BEARING ? 2 : 1;
        std::vector<double> z(m), W(m * m);                                // exactly what the kind reads
        z[0] = kind == APRILSAM_AMD_POLAR_BEARING ? 0.1 : 1.7;
        if (m == 2) { z[1] = 0.1; W = { 400.0, 30.0, 30.0, 900.0 }; } else W[0] = 400.0;
        double d2 = -1, S[4] = { -1, -1, -1, -1 };
        // Sigma = 0: S = W^-1 and d2 = r' W r
        CHECK(aprilsam_amd_debug_polar_gate(kind, pa, pb, z.data(), W.data(), zero.data(), &d2, S) == 0);
        const double ca = cos(pa[2]), sa = sin(pa[2]), dx = pb[0] - pa[0], dy = pb[1] - pa[1];
        const double want = asam::polar_cost(kind, z.data(), W.data(), ca * dx + sa * dy, -sa * dx + ca * dy);
        CHECK(std::fabs(d2 - want) <= 1e-12 * want && S[1] == S[2] && (m == 2 || (S[0] == 1.0 / W[0] && S[1] == 0 && S[3] == 0)));
        // a covariance only widens the gate
        double d2c = -1;
        CHECK(aprilsam_amd_debug_polar_gate(kind, pa, pb, z.data(), W.data(), eye.data(), &d2c, S) == 0 && d2c > 0 && d2c < d2);
        // rho == 0
        const double on[3] = { pa[0], pa[1], 2.0 };
        CHECK(aprilsam_amd_debug_polar_gate(kind, pa, on, z.data(), W.data(), eye.data(), &d2, S) == 1 && std::isnan(d2) && std::isnan(S[0]));
        // refusals
        CHECK(aprilsam_amd_debug_polar_gate(kind, nullptr, pb, z.data(), W.data(), eye.data(), &d2, S) == -13);
        CHECK(aprilsam_amd_debug_polar_gate(kind, pa, pb, z.data(), W.data(), nullptr, &d2, S) == -13);
        CHECK(aprilsam_amd_debug_polar_gate(kind, pa, pb, z.data(), W.data(), eye.data(), &d2, nullptr) == -13);
    }
    double d2 = 0, S[4];
    CHECK(aprilsam_amd_debug_polar_gate(0, pa, pb, pa, pa, eye.data(), &d2, S) == -13 && aprilsam_amd_debug_polar_gate(4, pa, pb, pa, pa, eye.data(), &d2, S) == -13);
    // what the two entry points judge before the device: two measurements, the first a range (z[0], W[0] read; NaN behind them)
    const char *why = nullptr;
    int kind[2] = { APRILSAM_AMD_POLAR_RANGE, APRILSAM_AMD_POLAR_RANGE_BEARING };
    double z[4] = { 1.0, NAN, 1.2, 0.3 }, W[8] = { 4.0, NAN, NAN, NAN, 5.0, 1.0, 1.0, 6.0 };
    CHECK(asam::polar_gate_args(2, kind, z, W, &why) == 0 && asam::polar_gate_args(0, nullptr, nullptr, nullptr, &why) == 0);
    kind[1] = 5; CHECK(asam::polar_gate_args(2, kind, z, W, &why) == -13 && why); kind[1] = APRILSAM_AMD_POLAR_RANGE_BEARING;
    z[3] = INFINITY; CHECK(asam::polar_gate_args(2, kind, z, W, &why) == -13); z[3] = 0.3;
    W[5] = NAN; CHECK(asam::polar_gate_args(2, kind, z, W, &why) == -13); W[5] = 1.0;
    W[0] = 0.0; CHECK(asam::polar_gate_args(2, kind, z, W, &why) == -12); W[0] = 4.0;
    W[6] = 1.5; CHECK(asam::polar_gate_args(2, kind, z, W, &why) == -12); W[6] = 1.0;
    W[5] = W[6] = 9.0; CHECK(asam::polar_gate_args(2, kind, z, W, &why) == -12);
    printf("ok\n");
    return 0;
}
