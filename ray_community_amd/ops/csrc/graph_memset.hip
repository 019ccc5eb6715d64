// Memset nodes of a captured HIP graph -> fill-kernel nodes.
//
// Work captured from libraries records hipMemsetAsync calls as memset nodes (PyTorch's reduction
// kernels clear their block semaphores that way, MIOpen's composable-kernel backward-data
// convolutions their output). Not every host replays such nodes: with the MI355X passed through
// to a virtual machine, a graph of fill(1) -> memset(0) -> copy copied zeros on its first replay
// and ones on the 39 after it, with no error, and the PPO learner's captured step drifted from
// its eager loop from the second update on. rca_graph_memsets_to_kernels rewrites the graph
// before it is instantiated: each memset node becomes a kernel node with the same dependencies
// and dependents that stores the same bytes, so a replay launches kernels only.
#include <vector>

#include "common.h"

// One memset (hipMemsetParams): `height` rows of `width` elements of `es` bytes (1, 2 or 4), rows
// `pitch` bytes apart, every element = the low `es` bytes of `value`. blockIdx.y strides over the
// rows; a row is stored as 16 B vectors over its 16 B-aligned middle and byte by byte over the
// (< 16 B) head and tail. No store leaves [row, row + width * es).
__global__ void __launch_bounds__(256) graph_fill_kernel(unsigned char* dst, unsigned value, int es, size_t width,
                                                         size_t height, size_t pitch) {
  const unsigned w = es == 1 ? (value & 0xffu) * 0x01010101u : es == 2 ? (value & 0xffffu) * 0x00010001u : value;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (size_t)gridDim.x * blockDim.x;
  for (size_t r = blockIdx.y; r < height; r += gridDim.y) {
    const uintptr_t b = (uintptr_t)dst + r * pitch, e = b + width * (size_t)es;
    uintptr_t a0 = (b + 15) & ~(uintptr_t)15;
    if (a0 > e) a0 = e;
    uintptr_t a1 = e & ~(uintptr_t)15;
    if (a1 < a0) a1 = a0;
    // the pattern repeats every 4 bytes from b: rotate it to the phase of the aligned middle
    const unsigned sh = (unsigned)((a0 - b) & 3) * 8;
    const unsigned wr = sh ? (w >> sh) | (w << (32 - sh)) : w;
    const u32x4 v = {wr, wr, wr, wr};
    const size_t chunks = (a1 - a0) >> 4;
    for (size_t i = tid; i < chunks; i += nthreads) reinterpret_cast<u32x4*>(a0)[i] = v;
    const size_t head = a0 - b, tail = e - a1;  // each < 16
    if (tid < head + tail) {
      const uintptr_t a = tid < head ? b + tid : a1 + (tid - head);
      *reinterpret_cast<unsigned char*>(a) = (unsigned char)(w >> (((a - b) & 3) * 8));
    }
  }
}

#define RCA_HIP(x)                      \
  do {                                  \
    hipError_t e_ = (x);                \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

// Replaces every memset node of `graph_handle` (a hipGraph_t: captured, not yet instantiated).
// *replaced: how many nodes were rewritten. Returns a hipError_t (0 = success); a memset of an
// element size other than 1, 2 or 4 bytes is hipErrorNotSupported.
RCA_API int rca_graph_memsets_to_kernels(void* graph_handle, int* replaced) {
  hipGraph_t graph = (hipGraph_t)graph_handle;
  *replaced = 0;
  size_t n = 0;
  RCA_HIP(hipGraphGetNodes(graph, nullptr, &n));
  std::vector<hipGraphNode_t> nodes(n);
  if (n) RCA_HIP(hipGraphGetNodes(graph, nodes.data(), &n));
  for (size_t i = 0; i < n; ++i) {
    hipGraphNodeType type;
    RCA_HIP(hipGraphNodeGetType(nodes[i], &type));
    if (type != hipGraphNodeTypeMemset) continue;
    hipMemsetParams p;
    RCA_HIP(hipGraphMemsetNodeGetParams(nodes[i], &p));
    if (p.elementSize != 1 && p.elementSize != 2 && p.elementSize != 4) return (int)hipErrorNotSupported;
    size_t nd = 0, nc = 0;
    RCA_HIP(hipGraphNodeGetDependencies(nodes[i], nullptr, &nd));
    std::vector<hipGraphNode_t> deps(nd);
    if (nd) RCA_HIP(hipGraphNodeGetDependencies(nodes[i], deps.data(), &nd));
    RCA_HIP(hipGraphNodeGetDependentNodes(nodes[i], nullptr, &nc));
    std::vector<hipGraphNode_t> children(nc);
    if (nc) RCA_HIP(hipGraphNodeGetDependentNodes(nodes[i], children.data(), &nc));

    unsigned char* dst = (unsigned char*)p.dst;
    unsigned value = p.value;
    int es = (int)p.elementSize;
    size_t width = p.width, height = p.height ? p.height : 1, pitch = p.pitch;
    void* args[] = {&dst, &value, &es, &width, &height, &pitch};
    const size_t chunks = (width * (size_t)es) / 16 + 1;
    size_t gx = (chunks + 255) / 256;
    hipKernelNodeParams kp = {};
    kp.func = (void*)graph_fill_kernel;
    kp.gridDim = dim3((unsigned)(gx < 2048 ? gx : 2048), (unsigned)(height < 65535 ? height : 65535), 1);
    kp.blockDim = dim3(256, 1, 1);
    kp.sharedMemBytes = 0;
    kp.kernelParams = args;
    kp.extra = nullptr;
    hipGraphNode_t fill;
    RCA_HIP(hipGraphAddKernelNode(&fill, graph, nd ? deps.data() : nullptr, nd, &kp));
    for (size_t c = 0; c < nc; ++c) RCA_HIP(hipGraphAddDependencies(graph, &fill, &children[c], 1));
    RCA_HIP(hipGraphDestroyNode(nodes[i]));
    ++*replaced;
  }
  return 0;
}
