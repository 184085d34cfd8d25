// What pg_adam_step decides on the host before it launches (posegen_amd/csrc/pg_optim_plan.h: check_tables, plan_entries,
// segments_of, entry_of_block) on the CPU under ASan + UBSan.  The tables are vectors of this program, so an entry written past
// the table or a lookup outside it shows as a heap overflow; a workgroup owned by the wrong tensor, or by none, as a failed check.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I posegen_amd/csrc optim_plan_asan.cpp
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "pg_optim_plan.h"

namespace {

using namespace pgop;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

float dummy[4];
char msg[320];

pg_adam_tensor tensor(long long count, int group = 0, int step = 1) {
    float* p = count > 0 ? dummy : nullptr;
    return pg_adam_tensor{p, p, p, p, count, group, step};
}

const pg_adam_group GROUPS[2] = {{1e-3, 0.9, 0.999, 1e-8, 0.0}, {1e-2, 0.5, 0.9, 1e-6, 0.1}};

int check(const std::vector<pg_adam_tensor>& t, int n_groups = 2, double max_norm = 1.0, const double* out = nullptr) {
    return check_tables((int)t.size(), t.data(), n_groups, GROUPS, max_norm, out, msg, sizeof msg);
}

// plans `counts`, then walks every segment boundary of every tensor (and every block when there are few): each block is owned by
// the entry whose range holds it, the ranges tile [0, nblocks) in order, and the entries are the non-empty tensors
long plan_and_walk(const std::vector<long long>& counts) {
    std::vector<pg_adam_tensor> t;
    for (size_t i = 0; i < counts.size(); ++i) t.push_back(tensor(counts[i], (int)(i % 2), 1 + (int)(i % 7)));
    CHECK(check(t) == 0);
    std::vector<Entry> tab(t.size());                            // exactly n_tensors entries: one more write is a heap overflow
    long long nblocks = -1;
    const int n = plan_entries((int)t.size(), t.data(), GROUPS, tab.data(), &nblocks);
    long long want_blocks = 0;
    int live = 0;
    for (long long c : counts) { want_blocks += (c + SEG - 1) / SEG; live += c > 0; }
    CHECK(n == live && nblocks == want_blocks);
    long long next = 0;
    long walked = 0;
    for (int e = 0; e < n; ++e) {
        const Entry& en = tab.data()[e];
        CHECK(en.count > 0 && en.first_block == next);
        const long long nb = segments_of(en.count);
        CHECK(nb >= 1 && (nb - 1) * SEG < en.count && en.count <= nb * SEG);
        CHECK(en.step_size > 0.0 && en.bc2_sqrt > 0.0 && en.bc2_sqrt <= 1.0);
        const long long probes[4] = {next, next + nb - 1, next + nb / 2, next + (nb > 1 ? 1 : 0)};
        for (long long b : probes) { CHECK(entry_of_block(tab.data(), n, b) == e); ++walked; }
        if (nblocks <= 4096)
            for (long long b = next; b < next + nb; ++b) { CHECK(entry_of_block(tab.data(), n, b) == e); ++walked; }
        next += nb;
    }
    CHECK(next == nblocks);
    return walked;
}

void check_refusals() {
    std::vector<pg_adam_tensor> one{tensor(5)};
    CHECK(check(one) == 0);
    CHECK(check(one, 2, PG_ADAM_NO_CLIP) == 0 && check(one, 2, 0.0) == 0);
    CHECK(check(one, 2, -2.0) != 0 && check(one, 2, std::numeric_limits<double>::quiet_NaN()) != 0);
    CHECK(check(one, 0) != 0 && check(one, PG_ADAM_MAX_GROUPS + 1) != 0);
    CHECK(check_tables(0, one.data(), 2, GROUPS, 1.0, nullptr, msg, sizeof msg) != 0);
    CHECK(check_tables(PG_ADAM_MAX_TENSORS + 1, one.data(), 2, GROUPS, 1.0, nullptr, msg, sizeof msg) != 0);
    CHECK(check_tables(1, nullptr, 2, GROUPS, 1.0, nullptr, msg, sizeof msg) != 0);
    CHECK(check_tables(1, one.data(), 2, nullptr, 1.0, nullptr, msg, sizeof msg) != 0);
    CHECK(check(one, 2, 1.0, reinterpret_cast<const double*>(reinterpret_cast<const char*>(dummy) + 4)) != 0);
    { auto t = one; t[0].group = 2; CHECK(check(t) != 0); t[0].group = -1; CHECK(check(t) != 0); }
    { auto t = one; t[0].step = 0; CHECK(check(t) != 0); }
    { auto t = one; t[0].count = -1; CHECK(check(t) != 0); }
    { auto t = one; t[0].grad = nullptr; CHECK(check(t) != 0); }
    { auto t = one; t[0].exp_avg = reinterpret_cast<float*>(reinterpret_cast<char*>(dummy) + 2); CHECK(check(t) != 0); }
    { auto t = one; t[0].count = std::numeric_limits<int64_t>::max(); CHECK(check(t) != 0); }      // (no overflow on the way to the refusal)
    {   // 2^31 - 1 segments are legal, one more is not
        std::vector<pg_adam_tensor> t{tensor(MAX_BLOCKS * SEG)};
        CHECK(check(t) == 0);
        t.push_back(tensor(1));
        CHECK(check(t) != 0);
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const pg_adam_group bad[] = {{-1e-3, 0.9, 0.999, 1e-8, 0.0}, {1e-3, 1.0, 0.999, 1e-8, 0.0}, {1e-3, 0.9, -0.1, 1e-8, 0.0},
                                 {1e-3, 0.9, 0.999, -1e-8, 0.0}, {1e-3, 0.9, 0.999, 1e-8, -0.1}, {nan, 0.9, 0.999, 1e-8, 0.0}};
    for (const pg_adam_group& q : bad) CHECK(check_tables(1, one.data(), 1, &q, 1.0, nullptr, msg, sizeof msg) != 0);
}

}  // namespace

int main() {
    check_refusals();
    long walked = 0;
    walked += plan_and_walk({0});
    walked += plan_and_walk({0, 0, 0});
    walked += plan_and_walk({1});
    walked += plan_and_walk({SEG - 1, SEG, SEG + 1});
    walked += plan_and_walk({0, 1, 0, SEG - 1, 0, 0, SEG, SEG + 1, 0, 2 * SEG + 7, 0});
    walked += plan_and_walk({(long long)SEG * 100000 + 1, 0, 5});
    walked += plan_and_walk({MAX_BLOCKS * SEG});
    {   // 4096 tensors: empty ones, one-element ones and ones around the segment size, interleaved
        std::vector<long long> c(PG_ADAM_MAX_TENSORS);
        const long long sizes[] = {0, 1, SEG - 1, SEG, SEG + 1, 3, 0, 5 * SEG};
        for (size_t i = 0; i < c.size(); ++i) c[i] = sizes[(i * 5 + i / 8) % 8];
        walked += plan_and_walk(c);
        walked += plan_and_walk(std::vector<long long>(PG_ADAM_MAX_TENSORS, 1));
        walked += plan_and_walk(std::vector<long long>(PG_ADAM_MAX_TENSORS, 0));
    }
    std::printf("%ld block lookups clean under ASan/UBSan\n", walked);
    return 0;
}
