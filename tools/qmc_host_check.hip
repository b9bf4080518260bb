// qmc_host_check.hip -- the host side of csrc/pem_qmc.hip under AddressSanitizer / UBSan, as a stand-alone program (no GPU needed):
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -Iinclude -Ihallthrusterpem_amd/csrc tools/qmc_host_check.hip hallthrusterpem_amd/csrc/pem_qmc.hip -o /tmp/qmc_host_check
//   /tmp/qmc_host_check
//
// Calls pem_sobol_directions into exactly 30 words for every dimension and every argument check of pem_sample_sobol_f64_dev with
// host arrays of exactly ndim entries, so that a read or write past either end is reported.  Exits 0 when every call returned what
// it should; the sanitizers abort on their own findings.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pem_common.h"
#include "pem_hip.h"
#include "pem_sobol_seq.h"

namespace pem {
char* error_buffer() {        // (the library's own lives in pem_kernels.hip)
    static thread_local char buf[512];
    return buf;
}
}  // namespace pem

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("FAILED line %d: %s  [%s]\n", __LINE__, #cond, pem::error_buffer()); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

static int sample(size_t n, uint64_t first, int ndim, int swap_dim, size_t ld, int bad_kind = -1, bool null_kind = false) {
    const size_t len = ndim > 0 && ndim <= PEM_SAMPLE_MAX_DIM ? (size_t)ndim : 1;
    std::vector<int32_t> kind(len, PEM_DIST_LOGUNIFORM);      // heap arrays of exactly ndim entries
    std::vector<double> a(len, 0.0), b(len, 1.0);
    if (bad_kind >= 0) kind[len - 1] = bad_kind;
    double* fake_out = reinterpret_cast<double*>(4096);       // never dereferenced by the host
    return pem_sample_sobol_f64_dev(n, first, 0x9E3779B97F4A7C15ull, 3u, 1, ndim, null_kind ? nullptr : kind.data(), a.data(), b.data(),
                                    swap_dim, fake_out, ld, nullptr);
}

int main() {
    for (int d = 0; d < PEM_SOBOL_DIMS; ++d) {
        std::vector<uint32_t> out(PEM_SOBOL_BITS, 0u);
        EXPECT(pem_sobol_directions(d, out.data()) == PEM_OK);
        for (int j = 0; j < PEM_SOBOL_BITS; ++j) EXPECT(out[j] == PEM_SOBOL_V[d][j] && out[j] != 0u && out[j] < (1u << PEM_SOBOL_BITS));
        EXPECT(out[0] == 1u << (PEM_SOBOL_BITS - 1));          // bit 0 of the Gray code switches the top bit in every dimension
    }
    std::vector<uint32_t> out(PEM_SOBOL_BITS, 0u);
    EXPECT(pem_sobol_directions(PEM_SOBOL_DIMS, out.data()) == PEM_ERR_INVALID_ARG);
    EXPECT(pem_sobol_directions(-1, out.data()) == PEM_ERR_INVALID_ARG);
    EXPECT(pem_sobol_directions(0, nullptr) == PEM_ERR_INVALID_ARG);

    const uint64_t end = 1ull << PEM_SOBOL_BITS;
    for (size_t n : {(size_t)10, (size_t)0}) {
        EXPECT(sample(n, 0, 0, -1, 16) == PEM_ERR_INVALID_ARG);
        EXPECT(sample(n, 0, -1, -1, 16) == PEM_ERR_INVALID_ARG);
        EXPECT(sample(n, 0, PEM_SAMPLE_MAX_DIM + 1, -1, 16) == PEM_ERR_INVALID_ARG);
        EXPECT(sample(n, 0, 3, -1, 16, -1, true) == PEM_ERR_INVALID_ARG);
        EXPECT(sample(n, 0, 3, -3, 16) == PEM_ERR_INVALID_ARG);
        EXPECT(sample(n, 0, 3, 3, 16) == PEM_ERR_INVALID_ARG);
        EXPECT(sample(n, 0, 17, -2, 16) == PEM_ERR_INVALID_ARG);
        EXPECT(sample(n, 0, 17, 16, 16) == PEM_ERR_INVALID_ARG);
        EXPECT(sample(n, 0, PEM_SAMPLE_MAX_DIM, PEM_SAMPLE_MAX_DIM - 1, 16) == PEM_ERR_INVALID_ARG);
        EXPECT(sample(n, 0, PEM_SAMPLE_MAX_DIM, -1, 16, 3) == PEM_ERR_INVALID_ARG);
        EXPECT(sample(n, 0, 1, -1, 16, 3) == PEM_ERR_INVALID_ARG);
        EXPECT(sample(n, end + 1, 3, -1, 16) == PEM_ERR_INVALID_ARG);
        EXPECT(sample(n, ~0ull - 4, 3, -1, 16) == PEM_ERR_INVALID_ARG);
    }
    EXPECT(sample(10, 0, 3, -1, 9) == PEM_ERR_INVALID_ARG);
    EXPECT(sample(10, end - 9, 3, -1, 16) == PEM_ERR_INVALID_ARG);
    EXPECT(sample(0, end, 3, -1, 0) == PEM_OK);
    EXPECT(sample(0, 0, PEM_SAMPLE_MAX_DIM, -1, 0) == PEM_OK);
    EXPECT(sample(0, 0, 16, 15, 0) == PEM_OK);
    // a well-formed call gets as far as the device: launched where there is one, PEM_ERR_NO_DEVICE where there is none -- not run here
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "qmc host checks passed", failures);
    return failures ? 1 : 0;
}
