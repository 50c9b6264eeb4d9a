// Fragment of kernels.hip (included there after the kernels, in front of the other launch fragments): how a launcher turns a run-time
// value into a template argument -- the callee is a generic lambda that reads it from its parameter's TYPE -- and the one grid clamp.
#pragma once
namespace {
// f(double{}) for EKF_STORE_F64 (0), f(float{}) for float tiles -- in f, decltype(ts) is the storage type -- then what every launcher
// returns: the error state the launches in f left
template <typename F> hipError_t with_storage(int storage, F &&f) {
    if (storage == 0) f(double{}); else f(float{});
    return hipGetLastError();
}

// f(std::true_type{}) or f(std::false_type{}): in f, decltype(b)::value is the flag
template <typename F> void with_bool(bool b, F &&f) { if (b) f(std::true_type{}); else f(std::false_type{}); }

// what a launcher hands a kernel that takes a recorded predict: the caller's, or zeros when none is folded in
PredictArgs predict_or_none(const PredictArgs *fused_predict) { return fused_predict ? *fused_predict : PredictArgs{}; }

// EKF_DOWNDATE_GRID (tuning builds; 0: no cap) bounds the grid of every pass kernel that walks its work list with a grid stride
unsigned clamp_grid(int64_t grid, int grid_cap) { return (unsigned)(grid_cap > 0 && grid > grid_cap ? grid_cap : grid); }
}  // namespace
