// How every kernel of libsert_hip.so is started (host side only): launch(kernel, grid, block, lds, stream, args...).
//   * The arguments are function arguments: each expression is evaluated once, and each value is converted to the
//     kernel's own parameter type.  A call passes EVERY parameter: a kernel pointer carries no default arguments.
//   * Exactly one of three paths is taken:
//       - a carried completion event is pending (CarriedEvent): hipExtLaunchKernel with that event as the kernel's stop
//         event.  An event bound to a kernel's OWN completion signal instead of a barrier packet queued behind it:
//         hipEventRecord stalls its queue for ~7 us on this system (the next dispatch waits for the command processor
//         to retire the barrier packet), the stop event of the kernel itself does not.  Not timed in in-step mode.
//       - the in-step timing hook is set (sert_timing_enable(m, 2), host/timing.inc): hipExtLaunchKernel with a (start,
//         stop) pair of the ring -- the kernel's own dispatch timestamps, no barrier packets, no serialisation.  A launch
//         that fails gives its slot back and goes out plain.
//       - otherwise the plain <<<>>> launch.
//     Both are one thread-local record: an untimed launch pays one predictable branch.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <tuple>
#include <type_traits>
#include <utility>

namespace sert {

// the source of event pairs in in-step mode: null outside a timing scope (ScopedTimer) of a model in that mode
struct InStepHook {
    bool (*take)(void* ctx, hipEvent_t* start, hipEvent_t* stop);   // false: no group is open, the launch is not timed
    void (*give_back)(void* ctx);                                    // the pair taken last: its launch did not happen
    void* ctx;
};

namespace detail {
struct LaunchState {
    hipEvent_t carried = nullptr;
    InStepHook hook = {nullptr, nullptr, nullptr};
};
inline LaunchState& launch_state() {
    static thread_local LaunchState s;
    return s;
}

template <typename... Formal, typename... Actual, size_t... I>
inline bool launch_with_events(void (*kernel)(Formal...), dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                               hipEvent_t start, hipEvent_t stop, std::index_sequence<I...>, Actual&... args) {
    std::tuple<std::remove_cv_t<Formal>...> tup{static_cast<std::remove_cv_t<Formal>>(args)...};
    void* ptrs[sizeof...(Formal) ? sizeof...(Formal) : 1] = {(void*)&std::get<I>(tup)...};
    return hipExtLaunchKernel((const void*)kernel, grid, block, ptrs, lds, stream, start, stop, 0) == hipSuccess;
}
}  // namespace detail

inline InStepHook& instep_hook() { return detail::launch_state().hook; }

// The first launch on this host thread inside the scope carries `ev` as its completion event (null: none does): the
// launch may sit several calls deep (launch_gemm).  A scope left without a launch leaves nothing armed.
class CarriedEvent {
public:
    explicit CarriedEvent(hipEvent_t ev) { detail::launch_state().carried = ev; }
    ~CarriedEvent() { detail::launch_state().carried = nullptr; }
    CarriedEvent(const CarriedEvent&) = delete;
};

template <typename... Formal, typename... Actual>
inline void launch(void (*kernel)(Formal...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, Actual&&... args) {
    static_assert(sizeof...(Formal) == sizeof...(Actual), "launch() passes every parameter of the kernel: a kernel pointer carries no default arguments");
    detail::LaunchState& ls = detail::launch_state();
    if (ls.carried) {
        const hipEvent_t ev = std::exchange(ls.carried, nullptr);
        (void)detail::launch_with_events(kernel, grid, block, lds, stream, nullptr, ev, std::index_sequence_for<Formal...>{}, args...);
        return;
    }
    if (ls.hook.take) {
        hipEvent_t start = nullptr, stop = nullptr;
        if (ls.hook.take(ls.hook.ctx, &start, &stop)) {
            if (detail::launch_with_events(kernel, grid, block, lds, stream, start, stop, std::index_sequence_for<Formal...>{}, args...)) return;
            ls.hook.give_back(ls.hook.ctx);
        }
    }
    kernel<<<grid, block, lds, stream>>>(static_cast<Formal>(std::forward<Actual>(args))...);
}

// A run-time k in LO..HI as a kernel's template argument: f(std::integral_constant<int, k>()), f a generic lambda that
// launches the instance.  false: k lies outside, f was not called.
template <int LO, int HI, typename F>
inline bool dispatch_int(int k, F&& f) {
    if constexpr (LO <= HI) {
        if (k == LO) { f(std::integral_constant<int, LO>()); return true; }
        return dispatch_int<LO + 1, HI>(k, f);
    }
    return false;
}

}  // namespace sert
