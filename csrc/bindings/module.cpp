// The torcheval_amd._C module.  Every binding unit (csrc/bindings/<family>.cpp) states each of its
// ops once: the function (it validates tensors, picks the current HIP stream of the tensor's
// device, forwards raw pointers to the launchers in csrc/kernels/*.hip and fails loudly on shapes /
// dtypes the kernels do not assume), then at the end of the file its pybind entry point, its
// dispatcher schema and its CUDA and Meta kernels.
#include <pybind11/pybind11.h>

#include "tea_runtime.h"

namespace py = pybind11;

// csrc/bindings/<family>.cpp
void tea_bind_counts(py::module_& m);
void tea_bind_sortscan(py::module_& m);
void tea_bind_reductions(py::module_& m);
void tea_bind_fid(py::module_& m);
void tea_bind_misc(py::module_& m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "torcheval_amd native ops: hand-written HIP/CDNA4 kernels for MI355X (gfx950)";
  m.attr("ARCH") = "gfx950";
  tea_bind_counts(m);
  tea_bind_sortscan(m);
  tea_bind_reductions(m);
  tea_bind_fid(m);
  tea_bind_misc(m);
  tea_register_runtime(m);
  tea_register_cpu_metrics(m);
  tea_register_rccl(m);
  tea_register_hostread(m);
}
