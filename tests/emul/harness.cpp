// TEST INFRASTRUCTURE (see shim/hip/hip_runtime.h): storage for the kernels' dynamic LDS, the fiber switch, and the emulated
// build of the kernel entry points (harness_entries.hpp) for the CPU tests.  Linked with every csrc/ source compiled for the
// host (build.py), so the emulated library also exports the whole C ABI of include/vp_hip.h.
#include <vector>
#include "act_io.hpp"

namespace vp {  // dynamic-LDS arrays of the kernels (per worker thread = per running workgroup): 160 KiB, the size of a CU's LDS
alignas(16) VP_EMU_LDS char smem[160 << 10];
alignas(16) VP_EMU_LDS unsigned char dw_smem[160 << 10];
alignas(16) VP_EMU_LDS unsigned char se_smem[64 << 10];
alignas(16) VP_EMU_LDS unsigned char bk_smem[64 << 10];
alignas(16) VP_EMU_LDS unsigned char det_smem[160 << 10];
alignas(16) VP_EMU_LDS float xs[40 << 10];
alignas(16) VP_EMU_LDS float sh[40 << 10];
alignas(16) VP_EMU_LDS float smem_f[12 << 10];   // ctx_exp_conv1_kernel (round 5)
}  // namespace vp

using namespace vp;

#ifndef VP_EMU_TSAN
// Work-item context switch of the fiber core (System V x86-64): callee-saved registers + stack pointer.  ucontext's
// swapcontext costs two sigprocmask system calls per switch; an emulated MFMA is 64 switches.
asm(R"(
.text
.globl emu_switch
.type emu_switch,@function
emu_switch:
  pushq %rbp
  pushq %rbx
  pushq %r12
  pushq %r13
  pushq %r14
  pushq %r15
  movq %rsp, (%rdi)
  movq %rsi, %rsp
  popq %r15
  popq %r14
  popq %r13
  popq %r12
  popq %rbx
  popq %rbp
  ret
.size emu_switch, .-emu_switch
)");
#endif

// launches run to completion before they return; every pointer is host memory
static hipError_t harness_done(hipError_t e) { return e; }
static const float* harness_ones() {
  static const std::vector<float> ones(4096, 1.0f);
  return ones.data();
}
static unsigned* harness_minmax_seed() {
  static thread_local unsigned mm[2];
  mm[0] = 0xFFFFFFFFu;
  mm[1] = 0u;
  return mm;
}

#include "harness_entries.hpp"
