// The 3 x 3 part of pg_pose_scores (posegen_amd/csrc/pg_pose_align.h) on the CPU, on poses read from stdin: what a wave of
// pg_posescore.hip does with one pose in PG_POSE_ALIGN_BEST and PG_POSE_ALIGN_ROTATION, with the sums taken over a vector instead of
// over lanes.  Built plain (g++ or clang++) it is the host test of the header against the numpy restatement (tests/pose_scores_ref.py);
// built with ASan + UBSan it shows an index outside T, s or the pose's vectors as a heap / stack overflow and a misuse of an
// uninitialised or out-of-range value as a failed run.  A NaN pose, a zero pose and rank-deficient poses must come back: no loop of
// the header depends on a value of the matrix.
//   stdin : n, then per pose J followed by J x 3 coordinates of pred and J x 3 of gt
//   stdout: per pose two lines (BEST, ROTATION) of 17 numbers: T[9] row-major, sum_s, s[3], det, d, scale, aligned
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I posegen_amd/csrc pose_align_asan.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pg_pose_align.h"

namespace {

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

void score(const std::vector<double>& p, const std::vector<double>& g, int J, bool rotation_only) {
    double mx[3] = {0, 0, 0}, my[3] = {0, 0, 0};
    for (int j = 0; j < J; ++j)
        for (int c = 0; c < 3; ++c) { mx[c] += g.at((size_t)j * 3 + c); my[c] += p.at((size_t)j * 3 + c); }
    for (int c = 0; c < 3; ++c) { mx[c] /= J; my[c] /= J; }
    std::vector<double> x0((size_t)J * 3), y0((size_t)J * 3);
    double ssx = 0.0, ssy = 0.0;
    for (int j = 0; j < J; ++j)
        for (int c = 0; c < 3; ++c) {
            const size_t i = (size_t)j * 3 + c;
            x0.at(i) = g.at(i) - mx[c]; y0.at(i) = p.at(i) - my[c];
            ssx += x0.at(i) * x0.at(i); ssy += y0.at(i) * y0.at(i);
        }
    const double nx = std::sqrt(ssx), ny = std::sqrt(ssy);
    double A[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < J; ++j)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) A[3 * r + c] += (x0.at((size_t)j * 3 + r) / nx) * (y0.at((size_t)j * 3 + c) / ny);
    const pgalign::Result f = pgalign::align(A, rotation_only);
    const double k = nx * f.sum_s;
    double sq = 0.0, al = 0.0;
    for (int j = 0; j < J; ++j) {
        double e = 0.0;
        for (int c = 0; c < 3; ++c) {
            double z = 0.0;
            for (int b = 0; b < 3; ++b) z += (y0.at((size_t)j * 3 + b) / ny) * f.T[3 * b + c];
            z = k * z + mx[c];
            e += (z - g.at((size_t)j * 3 + c)) * (z - g.at((size_t)j * 3 + c));
        }
        sq += e;
        al += std::sqrt(e);
    }
    // T is orthogonal whatever the matrix was, unless it holds a NaN
    bool finite = true;
    for (int i = 0; i < 9; ++i) finite = finite && std::isfinite(f.T[i]);
    if (finite)
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                double dot = 0.0;
                for (int q = 0; q < 3; ++q) dot += f.T[3 * r + q] * f.T[3 * c + q];
                CHECK(std::fabs(dot - (r == c ? 1.0 : 0.0)) < 1e-12);
            }
    CHECK(f.det == 1.0 || f.det == -1.0);
    for (int i = 0; i < 9; ++i) std::printf("%.17g ", f.T[i]);
    std::printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", f.sum_s, f.s[0], f.s[1], f.s[2], f.det, sq / ssx, f.sum_s * nx / ny, al / J);
}

}  // namespace

int main() {
    long n = 0;
    if (std::scanf("%ld", &n) != 1 || n < 0) { std::fprintf(stderr, "pose_align_asan: the number of poses is missing\n"); return 2; }
    for (long i = 0; i < n; ++i) {
        int J = 0;
        if (std::scanf("%d", &J) != 1 || J < 1 || J > 64) { std::fprintf(stderr, "pose_align_asan: pose %ld: J\n", i); return 2; }
        std::vector<double> p((size_t)J * 3), g((size_t)J * 3);
        for (std::vector<double>* v : {&p, &g})
            for (double& x : *v) {
                char word[64];
                if (std::scanf("%63s", word) != 1) { std::fprintf(stderr, "pose_align_asan: pose %ld is short\n", i); return 2; }
                x = std::strtod(word, nullptr);           // (reads nan and inf as well)
            }
        score(p, g, J, false);
        score(p, g, J, true);
    }
    std::printf("%ld poses done\n", n);
    return 0;
}
