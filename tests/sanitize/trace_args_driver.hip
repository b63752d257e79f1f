/* AddressSanitizer / UBSan driver for the argument checking of mpc_episode_trace_set_dev and mpc_episode_trace_dev, on the CPU.  Both entry points need a
 * handle, and a handle cannot be created without a device; so this program is ONE translation unit with the library -- it includes csrc/mpc_api.hip, which
 * makes struct mpc_handle visible -- and value-initialises a handle the way create_handle does, without any resource.  It walks only the refusal paths (and
 * attach / detach, which make no HIP call): nothing is launched, no device is needed.
 *
 *     hipcc --offload-arch=gfx950 -O1 -std=c++17 -Wno-unused-value -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
 *           -Xarch_host -fno-omit-frame-pointer -g -o build/sanitize/trace_args_driver tests/sanitize/trace_args_driver.hip && build/sanitize/trace_args_driver
 *
 * (device code is not instrumented; the compile is the library's own, minutes long, which is why no test of the suite builds it) */
#include "../../dynamic-obstacle-avoidance-mpc_amd/csrc/mpc_api.hip"
#include <cstdio>
#include <cstring>

static int bad = 0;

static void refused(int rc, const char *word, const char *what)
{
    if (rc != MPC_ERR_ARG || !strstr(mpc_last_error(), word)) {
        printf("NOT REFUSED as expected: %s -> %d, \"%s\" (wanted \"%s\")\n", what, rc, mpc_last_error(), word);
        bad++;
    }
}

int main()
{
    mpc_handle *h = new mpc_handle();           /* value-initialised, as create_handle leaves it before create_resources */
    h->max_batch = 4; h->device = 0;
    int32_t seed_row[8], slot_state[8], len[2], status[12], iters[12];
    double x[2 * 7 * 5], obst[2 * 7 * 5 * 4], u[2 * 6 * 2], pred[2 * 6 * 21 * 5];
    int32_t slot_seed[4], w[4];
    double x0[20], ob[80], X[4 * 105], u0[8];
    const mpc_episode_trace full = {seed_row, slot_state, len, x, obst, u, status, iters, pred};

    refused(mpc_episode_trace_set_dev(nullptr, 2, 6, &full), "null handle", "set: null handle");
    refused(mpc_episode_trace_dev(nullptr, 4, 0, slot_seed, x0, ob, X, u0, w, w, w, w, nullptr), "null handle", "trace: null handle");
    refused(mpc_episode_trace_dev(h, 4, MPC_TRACE_START, slot_seed, x0, ob, X, u0, w, w, w, w, nullptr), "no trace attached", "trace: nothing attached");
    refused(mpc_episode_trace_set_dev(h, -1, 6, &full), "rows", "set: rows < 0");
    refused(mpc_episode_trace_set_dev(h, 2, 0, &full), "max_steps", "set: max_steps < 1");
    refused(mpc_episode_trace_set_dev(h, 2, -5, &full), "max_steps", "set: max_steps < 0");
    const char *names[8] = {"seed_row", "slot_state", "len", "x is null", "obst", "u is null", "status", "iters"};
    for (int f = 0; f < 8; f++) {
        mpc_episode_trace t = full;
        void *zero = nullptr;
        memcpy(reinterpret_cast<char *>(&t) + f * sizeof(void *), &zero, sizeof(void *));      /* the struct is nine pointers */
        refused(mpc_episode_trace_set_dev(h, 2, 6, &t), names[f], names[f]);
    }
    refused(mpc_episode_trace_dev(h, 4, MPC_TRACE_STEP, slot_seed, x0, ob, X, u0, w, w, w, w, nullptr), "no trace attached", "trace: a refused attach attaches nothing");
    mpc_episode_trace nopred = full; nopred.pred = nullptr;
    if (mpc_episode_trace_set_dev(h, 2, 6, &nopred) != MPC_OK || h->trace_rows != 2 || h->trace_max_steps != 6 || h->trace.pred) { printf("attach without pred failed\n"); bad++; }
    refused(mpc_episode_trace_dev(h, 4, MPC_TRACE_STEP, slot_seed, x0, ob, X, nullptr, w, w, w, w, nullptr), "u0", "trace: STEP without u0");
    if (mpc_episode_trace_set_dev(h, 2, 6, &full) != MPC_OK || h->trace.pred != pred) { printf("attach failed\n"); bad++; }
    refused(mpc_episode_trace_dev(h, 0, MPC_TRACE_START, slot_seed, x0, ob, X, u0, w, w, w, w, nullptr), "slots", "trace: slots 0");
    refused(mpc_episode_trace_dev(h, 5, MPC_TRACE_START, slot_seed, x0, ob, X, u0, w, w, w, w, nullptr), "slots", "trace: slots > max_batch");
    refused(mpc_episode_trace_dev(h, 4, 2, slot_seed, x0, ob, X, u0, w, w, w, w, nullptr), "phase", "trace: phase 2");
    refused(mpc_episode_trace_dev(h, 4, -1, slot_seed, x0, ob, X, u0, w, w, w, w, nullptr), "phase", "trace: phase -1");
    refused(mpc_episode_trace_dev(h, 4, MPC_TRACE_START, nullptr, x0, ob, X, u0, w, w, w, w, nullptr), "slot_seed", "trace: null slot_seed");
    refused(mpc_episode_trace_dev(h, 4, MPC_TRACE_START, slot_seed, nullptr, ob, X, u0, w, w, w, w, nullptr), "x0", "trace: null x0");
    refused(mpc_episode_trace_dev(h, 4, MPC_TRACE_START, slot_seed, x0, nullptr, X, u0, w, w, w, w, nullptr), "obst", "trace: null obst");
    refused(mpc_episode_trace_dev(h, 4, MPC_TRACE_START, slot_seed, x0, ob, X, u0, w, w, nullptr, w, nullptr), "ep_flags", "trace: null ep_flags");
    refused(mpc_episode_trace_dev(h, 4, MPC_TRACE_START, slot_seed, x0, ob, X, u0, w, w, w, nullptr, nullptr), "ep_steps", "trace: null ep_steps");
    refused(mpc_episode_trace_dev(h, 4, MPC_TRACE_STEP, slot_seed, x0, ob, X, nullptr, w, w, w, w, nullptr), "u0", "trace: STEP without u0");
    refused(mpc_episode_trace_dev(h, 4, MPC_TRACE_STEP, slot_seed, x0, ob, X, u0, nullptr, w, w, w, nullptr), "status", "trace: STEP without status");
    refused(mpc_episode_trace_dev(h, 4, MPC_TRACE_STEP, slot_seed, x0, ob, X, u0, w, nullptr, w, w, nullptr), "iters", "trace: STEP without iters");
    refused(mpc_episode_trace_dev(h, 4, MPC_TRACE_STEP, slot_seed, x0, ob, nullptr, u0, w, w, w, w, nullptr), "pred", "trace: STEP without X while pred is attached");
    /* detach, both ways */
    if (mpc_episode_trace_set_dev(h, 0, 0, &full) != MPC_OK || h->trace_rows != 0 || h->trace.x) { printf("detach by rows == 0 failed\n"); bad++; }
    if (mpc_episode_trace_set_dev(h, 2, 6, &full) != MPC_OK || mpc_episode_trace_set_dev(h, 2, 6, nullptr) != MPC_OK || h->trace_rows != 0) { printf("detach by NULL failed\n"); bad++; }
    refused(mpc_episode_trace_dev(h, 4, MPC_TRACE_START, slot_seed, x0, ob, X, u0, w, w, w, w, nullptr), "no trace attached", "trace: detached");
    delete h;                                   /* (no resource was created: nothing for mpc_destroy to release) */
    printf("trace argument sanitizer driver: %d problems\n", bad);
    return bad ? 1 : 0;
}
