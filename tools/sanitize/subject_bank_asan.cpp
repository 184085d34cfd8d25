// The subject bank's swap logic (posegen_amd/csrc/pg_bank.h: bank_resize, bank_select -- what pg_set_subject_count and
// pg_select_subject run) on the CPU under ASan + UBSan.  "Device" memory is malloc'd here, so a subject that is dropped without
// its images being freed shows as a leak, and a subject read after a shrink as a use after free.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I posegen_amd/csrc subject_bank_asan.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "pg_bank.h"

namespace {

int g_live = 0;         // "device" allocations outstanding

void* dev_alloc(size_t n) { ++g_live; return std::malloc(n); }
void dev_free(void* p) { if (p) { --g_live; std::free(p); } }

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); std::exit(1); } } while (0)

// what pg_api.hip's release_subject does, with the frees of this program
void drop(Subject& s) {
    for (NetState& ns : s.net) {
        for (NetState::Slot& im : ns.img) { dev_free(im.d); im = {}; }
        dev_free(ns.d_codes); dev_free(ns.d_src); dev_free(ns.d_vwide);
        for (int32_t*& m : ns.d_map) { dev_free(m); m = nullptr; }
        ns = NetState();
    }
    dev_free(s.d_cut);
    s.d_cut = nullptr;
}

int make(Subject& s) {
    for (float& c : s.cut) c = 0.5f;
    s.d_cut = static_cast<float*>(dev_alloc(sizeof s.cut));
    return s.d_cut ? 0 : -2;
}

// a loaded model whose every value says which subject it is
void load(Subject& s, int id) {
    for (int w = 0; w < 2; ++w) {
        NetState& ns = s.net[w];
        ns.loaded = true;
        ns.host.assign(24, std::vector<float>(64 + id, (float)(10 * id + w)));
        ns.codes_host.assign(16 * (id + 2), (float)id);
        ns.fold_w.assign(32, (float)id);
        ns.n_codes = id + 1;
        for (int i : {(int)IMG_BIAS, (int)IMG_ONCHIP16 + PG_PREC_BF16, (int)IMG_C2}) {
            ns.img[i].bytes = 128 + id;
            ns.img[i].d = static_cast<uint8_t*>(dev_alloc(ns.img[i].bytes));
            std::memset(ns.img[i].d, id, ns.img[i].bytes);
        }
        ns.d_codes = static_cast<float*>(dev_alloc(64));
        ns.builds = 3;
    }
    for (float& c : s.cut) c = 1.0f + id;
    s.tau[0] = 20.f + id; s.tau[1] = 30.f + id;
    s.emb_set[0] = s.emb_set[1] = true;
    std::memcpy(s.d_cut, s.cut, sizeof s.cut);
}

void expect(const Subject& s, int id) {
    for (int w = 0; w < 2; ++w) {
        const NetState& ns = s.net[w];
        CHECK(ns.loaded && ns.host.size() == 24 && ns.host[7].size() == (size_t)(64 + id) && ns.host[7][3] == (float)(10 * id + w));
        CHECK(ns.n_codes == id + 1 && ns.codes_host.size() == (size_t)16 * (id + 2) && ns.fold_w[5] == (float)id);
        CHECK(ns.img[IMG_BIAS].d && ns.img[IMG_BIAS].bytes == (size_t)(128 + id) && ns.img[IMG_BIAS].d[100] == (uint8_t)id);
        CHECK(ns.img[IMG_C2].d[0] == (uint8_t)id && !ns.img[IMG_DIRECT].d && ns.builds == 3);
    }
    CHECK(s.cut[47] == 1.0f + id && s.tau[0] == 20.f + id && s.tau[1] == 30.f + id && s.emb_set[1]);
    CHECK(s.d_cut && s.d_cut[0] == 1.0f + id);
}

}  // namespace

int main() {
    {
        Subject act;            // the handle's own Subject part
        Bank b;
        CHECK(make(act) == 0);
        CHECK(bank_count(b) == 1);
        load(act, 0);
        bank_select(act, b, 0);                                 // one subject: nothing to do
        expect(act, 0);

        // grow to 4: subject 0 stays loaded and active, the new ones are empty with cutoffs of their own
        CHECK(bank_resize(act, b, 4, make, drop) == 0 && bank_count(b) == 4 && b.active == 0);
        expect(act, 0);
        for (int s = 1; s < 4; ++s) {
            bank_select(act, b, s);
            CHECK(b.active == s && !act.net[0].loaded && !act.emb_set[0] && act.d_cut && act.cut[0] == 0.5f && act.tau[0] == 20.f);
            load(act, s);
        }
        // every subject comes back as it was left, in any order, and its device pointers are its own
        const float* cuts[4];
        const uint8_t* imgs[4];
        for (int s : {2, 0, 3, 1, 1, 0}) {
            bank_select(act, b, s);
            expect(act, s);
            cuts[s] = act.d_cut; imgs[s] = act.net[1].img[IMG_C2].d;
        }
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j) CHECK(cuts[i] != cuts[j] && imgs[i] != imgs[j]);
        // a selection allocates nothing and frees nothing
        const int live = g_live;
        for (int k = 0; k < 1000; ++k) bank_select(act, b, k % 4);
        CHECK(g_live == live);
        for (int s = 0; s < 4; ++s) { bank_select(act, b, s); expect(act, s); CHECK(act.d_cut == cuts[s]); }

        // grow again with subject 2 active: everything kept
        bank_select(act, b, 2);
        CHECK(bank_resize(act, b, 6, make, drop) == 0 && bank_count(b) == 6 && b.active == 2);
        expect(act, 2);
        bank_select(act, b, 3); expect(act, 3);
        bank_select(act, b, 5); CHECK(!act.net[0].loaded);
        load(act, 5);

        // shrink to 3 with subject 1 active: 3, 4 (empty), 5 are freed, the others untouched
        bank_select(act, b, 1);
        const int before = g_live;
        CHECK(bank_resize(act, b, 3, make, drop) == 0 && bank_count(b) == 3 && b.active == 1);
        CHECK(g_live == before - 2 * (2 * 4 + 1) - 1);          // two loaded subjects (8 net allocations + d_cut) and an empty one
        expect(act, 1);
        bank_select(act, b, 0); expect(act, 0);
        bank_select(act, b, 2); expect(act, 2);

        // a failing allocation while growing leaves the bank at the size reached
        int calls = 0;
        auto flaky = [&](Subject& s) { return ++calls == 2 ? -2 : make(s); };
        CHECK(bank_resize(act, b, 6, flaky, drop) == -2 && bank_count(b) == 4 && b.active == 2);
        expect(act, 2);

        // back to one subject (subject 0 active): the bank's vector goes, subject 0 stays whole
        bank_select(act, b, 0);
        CHECK(bank_resize(act, b, 1, make, drop) == 0 && bank_count(b) == 1 && b.parked.empty());
        expect(act, 0);
        // and up again from one
        CHECK(bank_resize(act, b, 2, make, drop) == 0);
        bank_select(act, b, 1); load(act, 1);
        bank_select(act, b, 0); expect(act, 0);
        bank_select(act, b, 1); expect(act, 1);

        // what pg_destroy does
        drop(act);
        for (Subject& s : b.parked) drop(s);
    }
    CHECK(g_live == 0);
    std::puts("subject bank clean under ASan/UBSan");
    return 0;
}
