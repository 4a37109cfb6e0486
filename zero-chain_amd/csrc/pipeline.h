// libzkamd, zk_pipeline: a stream of statement batches.  zk_transfer_prove_batch overlaps the witnesses of chunk k + 1 with the
// GPU work of chunk k INSIDE one call; a service that proves batch after batch wants the same overlap ACROSS calls.  submit()
// queues the chunks of a batch and returns; the lanes - worker threads, each with its own workspaces and streams over the
// same tables - take them (pipeline_lanes.h), each making the witnesses of its next chunk (ChunkWitness, statement_route.h)
// beside the proving of its current one; wait() returns when everything submitted so far is proved.  With the witness
// kernels several lanes keep several chunks in flight: the sort / reduction / fold / witness phases of one beside the
// accumulation of another.  With the host calculator (ZKAMD_WITNESS=host) there is lane 0 alone, on the caller's handles:
// its one helper thread fills the halves of the circuit's pinned host_z.  Part of zkamd.cpp's translation unit.
#pragma once
#include <optional>
#include "pipeline_lanes.h"
#include "statement_route.h"

struct zk_pipeline {
    static constexpr int MAX_LANES = 4;
    // the handles of each lane: lane 0 the caller's own, lanes 1 .. (ZKAMD_PIPELINE_LANES, default 2) clones that borrow the tables
    zk_params* Pl[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
    zk_r1cs* Rl[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr};
    std::thread t_lane[MAX_LANES];
    int n_lanes = 1;    // lanes started at create
    size_t chunk = 0;   // (proofs per launch set: ProveTunables, at zk_pipeline_create)
    bool host = false;  // the witness engine (witness_on_host, at zk_pipeline_create)
    zkpipe::LaneQueue Q;
};

namespace {

// what a lane of lane_run does, on the GPU
struct PipelineLane {
    zk_pipeline* const L;
    const int lane;
    std::optional<ChunkWitness> wit;   // over the lane's own circuit handle, once the lane has its context

    zk_status open() {
        g_lane = lane;
        ZK_TRY(use_device(L->Pl[lane]->key.device));
        wit.emplace(L->Rl[lane], STATEMENT_ROUTES[zkpairs::TRANSFER], L->host, L->chunk, false);
        return ZK_OK;
    }
    zk_status start(const zkpipe::Job& j, int slot) {
        const zk_status rc = guarded([&] { return wit->start(j.st, j.n, slot, j.index_base); });
        // test hook: a lane beyond the first behaves as if its workspaces did not fit (tests/test_gpu_parity.py)
        if (lane > 0 && hook_env("ZKAMD_INJECT_LANE_OOM")) return fail(ZK_ERR_OUT_OF_MEMORY, "injected: lane workspaces do not fit");
        return rc;
    }
    zk_status ready(const zkpipe::Job& j, int slot) {
        return guarded([&] { return wit->ready(j.n, slot, j.index_base); });
    }
    zk_status prove(const zkpipe::Job& j, int slot) {   // (as prove_statements does)
        return guarded([&] {
            const uint8_t* host_z = wit->host_z(slot);
            return host_z ? prove_batch_witness(L->Pl[lane], L->Rl[lane], j.n, host_z, ZK_FR_MONTGOMERY, j.rs, j.out, true)
                          : prove_from_z(L->Pl[lane], L->Rl[lane], j.n, slot, j.rs, j.out, true);
        });
    }
    // (the helper thread of a started job reads the caller's statements: joined before the failed job is counted.  The host engine
    //  is one lane, so its stream fails only in a turn of this lane, which comes through here: no started job is dropped unjoined)
    void drain_device() {
        wit->drain();
        (void)hipDeviceSynchronize();
    }
    void release() {   // borrowed tables stay with the original, the lane's own buffers are freed
        wit.reset();
        delete L->Pl[lane];
        delete L->Rl[lane];
        L->Pl[lane] = nullptr;
        L->Rl[lane] = nullptr;
    }
    std::string message() const { return g_err; }
};

}  // namespace
