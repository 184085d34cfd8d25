// pg_modules.h -- the one way a module keeps state on the renderer handle: a table with one typed slot per module.  Host-only and
// free of HIP calls, so that the slot logic compiles into a plain C++ program (tools/sanitize/module_slots_asan.cpp, built with the
// address and undefined-behaviour sanitisers).
//
// A module's state struct derives from ModuleState, names its slot (`static constexpr ModuleSlot SLOT`) and frees what it owns in
// its destructor: a member added to a state is released where it is declared, and nothing else lists the modules' members.
#pragma once
#include <memory>
#include <new>
#include <type_traits>

struct ModuleState { virtual ~ModuleState() = default; };

// (the order in which a handle's states are destroyed)
enum ModuleSlot { MOD_TRAIN, MOD_MESH, MOD_POSEOPT, MOD_BATCH, MOD_METRICS, MOD_POSESCORE, MOD_SMPL, MOD_KPLOSS, MOD_TRAINLOSS,
                  MOD_REGRESSOR, MOD_FRAMES, MOD_SCENE, MOD_DISC, MOD_HMR, MOD_OPTIM, MOD_GEN, MOD_COUNT };

struct Modules {
    std::unique_ptr<ModuleState> slot[MOD_COUNT];

    // the state if a call has created it, else null: for the calls that only read what an earlier one left
    template <class S> S* peek() const {
        static_assert(std::is_base_of<ModuleState, S>::value, "a module's state derives from ModuleState");
        return static_cast<S*>(slot[S::SLOT].get());
    }
    // the state, created on first use; null when out of memory
    template <class S> S* get() {
        if (!slot[S::SLOT]) slot[S::SLOT].reset(new (std::nothrow) S());
        return peek<S>();
    }
    // destroys the states in slot order (the members' own destructors would run in the reverse one)
    void clear() {
        for (auto& s : slot) s.reset();
    }
    ~Modules() { clear(); }
};
