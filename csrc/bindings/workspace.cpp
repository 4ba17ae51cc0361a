// The per-stream workspace cache declared in tea_torch.h: the one definition, so every binding
// unit sees the same buffers.
#include <mutex>
#include <unordered_map>

#include "tea_torch.h"

namespace tea_torch {

void* workspace(const Tensor& like, hipStream_t stream, int64_t bytes, bool zeroed, int slot, int64_t* capacity) {
  static std::mutex mu;
  // process-lifetime (never destroyed): no device free from a static destructor at exit, after
  // the HIP runtime or an attached profiler has already shut down
  static auto& cache = *new std::unordered_map<uint64_t, Tensor>();
  // stream handles are user-space addresses (below 2^47): bits 48.. are free for the rest
  const uint64_t key = (static_cast<uint64_t>(like.device().index()) << 56) ^
                       (static_cast<uint64_t>(zeroed) << 55) ^ (static_cast<uint64_t>(slot) << 48) ^
                       reinterpret_cast<uint64_t>(stream);
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find(key);
  if (it == cache.end() || it->second.numel() < bytes) {
    const auto opts = at::TensorOptions().dtype(at::kByte).device(like.device());
    const int64_t size = std::max<int64_t>(bytes, 1 << 16);
    Tensor ws = zeroed ? at::zeros({size}, opts) : at::empty({size}, opts);
    if (it == cache.end()) it = cache.emplace(key, ws).first;
    else it->second = ws;
  }
  if (capacity) *capacity = it->second.numel();
  return it->second.data_ptr();
}

}  // namespace tea_torch
