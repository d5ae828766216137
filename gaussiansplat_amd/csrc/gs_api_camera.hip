// gs_api_camera.hip -- gs_backward_camera: the gradient of the frame's loss with respect to the arguments of gs_set_camera, from the rows of
// 2-D gradient sums the frame's colour backward left (c->g2d), the resident model and c->cam.  The kernels are gs_camera.hip's, the statement
// gs_camera_grad.h's.  The call reads the frame and writes only `out` and a buffer of its own (gs_ctx::camera_partials: 256 bytes for the
// 40 floats of a GS_MEM_HOST call, then one row of 40 doubles per workgroup): image, transmittance, g2d and g2d_clean, dpc, the stage, the
// view slot's history and the stage timers stay what they were.  Every refusal is made before anything is enqueued or allocated.
#include "gs_ctx.h"
#include "gs_camera_grad.h"

using Stage = gs_ctx::Stage;

static_assert(GS_CAMERA_GRAD_FLOATS == GS_CAMERA_GRAD_VALUES, "the ABI's 40 floats are the statement's 40 values");
#define GS_CAMERA_OUT_BYTES 256           // the staged floats in front of the partial rows (which keep their 16-byte alignment)

extern "C" {

int gs_backward_camera(gs_ctx *c, float *out, int mem) {
    if (!c) return GS_ERR_INVALID;
    if (const int rc = need_3d(c, "gs_backward_camera")) return rc;
    if (!out) return fail(c, GS_ERR_INVALID, "gs_backward_camera: NULL argument");
    if (const int rc = need_mem(c, "gs_backward_camera", mem)) return rc;
    if (const int rc = need_stage(c, Stage::COMPOSITE_ADJOINT,
                                  "gs_backward_camera: gs_backward first (the frame's colour backward leaves the rows this call reads; a call that steps the model drops them)")) return rc;
    if (bind_device(c)) return GS_ERR_HIP;
    const int64_t rows = gs_camera_grad_rows(c->n);
    HIPCHK(c, c->camera_partials.ensure(GS_CAMERA_OUT_BYTES + sizeof(double) * GS_CAMERA_GRAD_VALUES * (size_t)rows));
    float *stage = c->camera_partials.as<float>();
    GsCameraGradArgs a{};
    model_head(c, a);                                                      // the active degree on the stored rows, as the backward has it
    c->rows(c->g2d).into(a);
    a.partials = reinterpret_cast<double *>(c->camera_partials.as<char>() + GS_CAMERA_OUT_BYTES);
    HIPCHK(c, gs_launch_camera_grad(a, c->cam, mem == GS_MEM_HOST ? stage : out, c->stream));
    if (mem == GS_MEM_HOST) {
        HIPCHK(c, hipMemcpyAsync(out, stage, sizeof(float) * GS_CAMERA_GRAD_FLOATS, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return GS_OK;
}

}  // extern "C"
