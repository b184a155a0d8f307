// Sanitizer driver for the host BCS recurrence (fsnap_bcs_gram in fsnap_solve.cpp): sparse-truth systems of correlated columns
// (Gaussian columns mixed by I + 2 N / sqrt(K), so that the recurrence goes through deletions) at K = 1 ... 160,
// both deletion modes, max_active = 1, 2, K / 2 and K (so that additions are blocked and the output arrays are exactly full),
// itermax = 1 and 60, sigma2 given and from scale, a dead column and an all-dead system.  CPU only (GPU AddressSanitizer is
// not available on the pool):
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -mavx2 -mfma -pthread -I fitsnap_amd/csrc -I include \
//       tools/bcs_host_sanitize.cpp fitsnap_amd/csrc/fsnap_rowspace_host.cpp fitsnap_amd/csrc/fsnap_solve.cpp -o /tmp/bcs_san && /tmp/bcs_san
// The output arrays are allocated at exactly the documented sizes, so a write past one of them is reported.  As committed: 544
// runs, 22 deletions, no report.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "fsnap_hip.h"

int main() {
    std::mt19937_64 g(11);
    std::normal_distribution<double> N(0, 1);
    long runs = 0, deletions = 0, failed = 0;
    for (int K : {1, 2, 3, 7, 33, 64, 65, 144, 160}) {
        const int m = 3 * K + 40;
        std::vector<double> A((size_t)m * K), y(m), truth(K, 0.0);
        {
            std::vector<double> X((size_t)m * K), M((size_t)K * K);
            for (auto& v : X) v = N(g);
            for (int a = 0; a < K; ++a)
                for (int b = 0; b < K; ++b) M[(size_t)a * K + b] = (a == b ? 1.0 : 0.0) + 2.0 * N(g) / std::sqrt((double)K);
            for (int i = 0; i < m; ++i)
                for (int b = 0; b < K; ++b) {
                    double v = 0.0;
                    for (int a = 0; a < K; ++a) v += X[(size_t)i * K + a] * M[(size_t)a * K + b];
                    A[(size_t)i * K + b] = v;
                }
        }
        for (int j = 0; j < K; j += 5) truth[j] = 2.0 * N(g);
        for (int i = 0; i < m; ++i) {
            double s = 0.4 * N(g);
            for (int j = 0; j < K; ++j) s += A[(size_t)i * K + j] * truth[j];
            y[i] = s;
        }
        std::vector<double> Q((size_t)K * K, 0.0), q(K, 0.0), ref(K);
        double y2 = 0.0, sy = 0.0;
        for (int i = 0; i < m; ++i) {
            y2 += y[i] * y[i];
            sy += y[i];
            for (int a = 0; a < K; ++a) {
                q[a] += A[(size_t)i * K + a] * y[i];
                for (int b = 0; b < K; ++b) Q[(size_t)a * K + b] += A[(size_t)i * K + a] * A[(size_t)i * K + b];
            }
        }
        for (int deletion : {FSNAP_BCS_REFERENCE, FSNAP_BCS_EXACT})
            for (int ma : {1, 2, K / 2, K})
                for (int itermax : {1, 60})
                    for (int variant = 0; variant < 4; ++variant) {
                        if (ma < 1 || ma > K) continue;
                        for (int j = 0; j < K; ++j) ref[j] = Q[(size_t)j * K + j];
                        if (variant == 2) ref[0] = 0.0;                                  // a dead column
                        if (variant == 3) for (auto& v : ref) v = 0.0;                   // no live column
                        const double sigma2 = variant == 1 ? 0.05 : 0.0;
                        std::vector<double> coef(K), alpha(ma), mu(ma), err(ma), Sig((size_t)ma * ma), info(6);
                        std::vector<int32_t> active(ma), picks((size_t)2 * itermax);
                        const int rc = fsnap_bcs_gram(K, Q.data(), q.data(), y2, sy, (double)m, ref.data(), sigma2, 1e-2, 1e-18, itermax, ma,
                                                      deletion, coef.data(), active.data(), alpha.data(), mu.data(), err.data(), Sig.data(),
                                                      picks.data(), info.data());
                        if (rc != FSNAP_OK) {
                            printf("K=%d ma=%d itermax=%d variant=%d: status %d\n", K, ma, itermax, variant, rc);
                            return 1;
                        }
                        ++runs;
                        failed += info[1] == 1.0;
                        for (int t = 0; t < itermax; ++t) deletions += picks[2 * t + 1] == 2;
                    }
    }
    printf("%ld runs, %ld deletions, %ld with status 1: no sanitizer report\n", runs, deletions, failed);
    return 0;
}
