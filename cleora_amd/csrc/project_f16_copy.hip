// project_f16_copy.hip — the COPY instantiations of project_f16_kernel (project_f16.hip): the whitened loop's projection that also
// writes the f16 gather copy of its output (CLEORA_F_GATHER_F16).  A translation unit of its own so that it can be compiled without
// packed f32 arithmetic (build.sh) while project_f16.hip's object stays what it was.
#define PF_COPY_TU 1
#include "project_f16.hip"
