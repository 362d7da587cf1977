// The launch path of the host side (launch.cpp) and what batch.cpp, context_cache.cpp and regressor.cpp share with it.  Host .cpp files only.
#pragma once

#include "fwgpu_internal.h"

#pragma GCC visibility push(hidden)  // shared among the library's host files, not exported from it
namespace fwgpu {

// Which example kernel a launch is planned for: the regressor's own setting (fwgpu_debug_set_kernel_version), the generic kernel (peer-sharded
// launches: it carries the owner lookup, kernels.hip ffm_w_base / lr_base) or the resident kernel (packed launches: the packed gather exists there only)
enum class KernelChoice { kOwn, kGeneric, kResident };

// A planned launch of the example kernels: the resolved parameters, the workgroup size, and the grid (1: one workgroup walks the batch,
// FWGPU_MODE_SEQUENTIAL; 0: "what the device keeps resident", launch_persistent)
struct LaunchPlan {
    KernelParams p;
    uint32_t threads;
    uint32_t grid;
};

KernelParams make_params(const fwgpu_regressor *r, const fwgpu_batch *b, int update, KernelChoice kernel = KernelChoice::kOwn);
// launch shape of a batch: workgroup size, LDS copy of the LUT or not (settles p.window / p.chain / p.lut_global).  FWGPU_OK, or the code of a
// refusal with its reason in *why; neither planner touches the error string.
int plan_launch(const fwgpu_regressor *r, const fwgpu_batch *b, int mode, int update, KernelChoice kernel, LaunchPlan &plan, const char **why);
// ... of a predict-only batch whose deep head runs afterwards, for the whole batch (run_batch_head_predict)
int plan_head_inputs(const fwgpu_regressor *r, const fwgpu_batch *b, LaunchPlan &plan, const char **why);

// (`route`: where fwgpu_learn_batch records the path the launch took -- fwgpu_debug_last_route; the single-example calls pass none)
int run_batch(fwgpu_regressor *r, fwgpu_batch *b, int mode, int update, hipStream_t stream, int32_t *route = nullptr);
// Why the requests kernels (requests.hip) do not serve this regressor / batch shape, or NULL.  Asked when a set is attached and again at every launch.
const char *requests_refusal(const fwgpu_regressor *r, const fwgpu_batch *b);
// the regressor's host-mapped batch of one example, and its prediction once the launch has finished
int ensure_one(fwgpu_regressor *r, uint32_t n_lr, uint32_t n_ffm);
int one_prediction(fwgpu_regressor *r, float *prediction);

// context_cache.cpp
void requests_detach(fwgpu_batch *b);
bool cache_is_stale(const fwgpu_regressor *r, const fwgpu_block_cache *c);
extern const char *const kStaleCache;

// regressor.cpp
float initial_acc(int optimizer, float init_acc);

}  // namespace fwgpu
#pragma GCC visibility pop
