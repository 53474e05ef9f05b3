// fma_chain.cpp -- the trailing update of the column walk, W -= E @ U, per element a k-ordered fmaf chain from 0 and one
// subtraction, in exact fp32 (numpy has no fused multiply-add).  Built by tests/iq4_gptq_spec.py with
// g++ -O1 -ffp-contract=off.  stdin: int64 R, K, N, then E [R, K], U [K, N], W [R, N] as fp32; stdout: W [R, N].
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

int main() {
    int64_t h[3];
    if (fread(h, sizeof(int64_t), 3, stdin) != 3) return 2;
    const int64_t R = h[0], K = h[1], N = h[2];
    std::vector<float> E(R * K), U(K * N), W(R * N);
    if (fread(E.data(), 4, E.size(), stdin) != E.size() || fread(U.data(), 4, U.size(), stdin) != U.size() ||
        fread(W.data(), 4, W.size(), stdin) != W.size())
        return 2;
    for (int64_t r = 0; r < R; ++r)
        for (int64_t n = 0; n < N; ++n) {
            float acc = 0.0f;
            for (int64_t k = 0; k < K; ++k) acc = fmaf(E[r * K + k], U[k * N + n], acc);
            W[r * N + n] = W[r * N + n] - acc;
        }
    return fwrite(W.data(), 4, W.size(), stdout) == W.size() ? 0 : 2;
}
