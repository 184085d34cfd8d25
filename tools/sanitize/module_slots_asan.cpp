// The handle's table of module states (posegen_amd/csrc/pg_modules.h: Modules::peek, get, clear -- what pg_state and pg_destroy
// run) on the CPU under ASan + UBSan.  Each state here owns a heap block, so a slot that is dropped without its destructor shows as
// a leak and one that is destroyed twice as a double free; the destructors log their slots, which gives the order.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I posegen_amd/csrc module_slots_asan.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pg_modules.h"

namespace {

std::vector<int> g_log;         // the slots of the states destroyed so far, in order

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

template <ModuleSlot WHERE>
struct Owner : ModuleState {
    static constexpr ModuleSlot SLOT = WHERE;
    int* block = new int[16]();
    ~Owner() override { g_log.push_back(SLOT); delete[] block; }
};
using TrainLike = Owner<MOD_TRAIN>;
using BatchLike = Owner<MOD_BATCH>;
using FramesLike = Owner<MOD_FRAMES>;
using SceneLike = Owner<MOD_SCENE>;

bool all_empty(const Modules& m) {
    for (const auto& s : m.slot) if (s) return false;
    return true;
}

}  // namespace

int main() {
    {
        Modules m;
        CHECK(all_empty(m));
        CHECK(!m.peek<TrainLike>() && !m.peek<SceneLike>());     // peek creates nothing
        CHECK(all_empty(m));

        // created on first use, the same object from then on, and only its own slot
        SceneLike* sc = m.get<SceneLike>();
        CHECK(sc && m.get<SceneLike>() == sc && m.peek<SceneLike>() == sc);
        CHECK(m.slot[MOD_SCENE].get() == sc && !m.peek<TrainLike>() && !m.peek<BatchLike>());
        sc->block[3] = 7;
        // in an order other than the slots'
        FramesLike* fr = m.get<FramesLike>();
        TrainLike* tr = m.get<TrainLike>();
        BatchLike* ba = m.get<BatchLike>();
        CHECK(fr && tr && ba && m.get<TrainLike>() == tr && m.get<SceneLike>() == sc && sc->block[3] == 7);

        // clear: slot order, every slot null
        m.clear();
        CHECK((g_log == std::vector<int>{MOD_TRAIN, MOD_BATCH, MOD_FRAMES, MOD_SCENE}));
        CHECK(all_empty(m) && !m.peek<TrainLike>());
        // a second one does nothing
        m.clear();
        CHECK(g_log.size() == 4 && all_empty(m));

        // and the table is usable again
        g_log.clear();
        BatchLike* again = m.get<BatchLike>();
        CHECK(again && m.peek<BatchLike>() == again);
        m.clear();
        CHECK((g_log == std::vector<int>{MOD_BATCH}));
    }
    g_log.clear();
    {   // a table that goes out of scope with live slots frees them, in slot order as well
        Modules m;
        CHECK(m.get<SceneLike>() && m.get<BatchLike>() && m.get<TrainLike>());
    }
    CHECK((g_log == std::vector<int>{MOD_TRAIN, MOD_BATCH, MOD_SCENE}));
    std::puts("module slots clean under ASan/UBSan");
    return 0;
}
