// The queue and the lane loop of zk_pipeline (csrc/pipeline_lanes.h) without a GPU: fake lanes whose steps take a seeded few
// hundred microseconds, so that the schedules of the lanes vary from seed to seed.  Built with -fsanitize=thread and run by
// tests/test_pipeline_lanes.py.  Every scenario checks that each job is proved exactly once - by the lane that finished it,
// after whatever lanes handed it back - and the outcome listed with it.  Exit status 0: all held.
#include <stdio.h>
#include <stdlib.h>
#include <atomic>
#include <chrono>
#include <functional>
#include <thread>
#include <vector>
#include "../zero-chain_amd/csrc/pipeline_lanes.h"

using zkpipe::Job;
using zkpipe::LaneQueue;

namespace {

int g_failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            g_failures++;                                 \
            fprintf(stderr, "FAILED %s: ", #cond);        \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, " (line %d)\n", __LINE__);    \
        }                                                 \
    } while (0)

constexpr int MAX_JOBS = 8192;
constexpr int MAX_ROUNDS = 500;   // (a scenario that waits for a lane to meet its fault submits again, this often at the most)
std::atomic<int> g_ahead_oom{0};    // retirements at the start of a job taken ahead, over the whole run

// what the fakes of one pipeline record, per job (a job is its index_base) and per lane
struct Record {
    std::atomic<int> started[MAX_JOBS], proved[MAX_JOBS];
    std::atomic<int> released[4], drained[4], proved_by_lane[4];
    std::atomic<int> wit_done[MAX_JOBS];                     // HostFakeLane: the helper thread has made the job's witnesses
    std::atomic<int> beside{0}, not_beside{0}, not_ready{0};   // ... and what its prove() / ready() found
    Record() {
        for (auto& a : wit_done) a = 0;
        for (auto& a : proved_by_lane) a = 0;
        for (auto& a : started) a = 0;
        for (auto& a : proved) a = 0;
        for (auto& a : released) a = 0;
        for (auto& a : drained) a = 0;
    }
};

// which step of which lane fails, and how
struct Plan {
    int no_context_lane = -1;                  // open() fails on this lane
    int oom_lane_mask = 0;                     // these lanes run out of memory ...
    int oom_at_start = 1;                      // ... at their n-th start (1: their first, 2: the start of the job taken ahead)
    int bad_job = -1;                          // ready() of this job reports a malformed statement
    bool host = false;                         // the lanes are HostFakeLanes
};

struct FakeLane {
    Record& rec;
    const Plan& plan;
    const int lane;
    uint64_t rng;
    int n_starts = 0;
    bool oom = false;
    std::string msg;

    void step() {   // a seeded 50 .. 300 us
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        std::this_thread::sleep_for(std::chrono::microseconds(50 + (rng >> 33) % 250));
    }
    zk_status fail(zk_status st, const std::string& m) {
        msg = m;
        return st;
    }
    zk_status open() { return lane == plan.no_context_lane ? fail(ZK_ERR_DEVICE, "no context") : ZK_OK; }
    zk_status start(const Job& j, int) {
        step();
        rec.started[j.index_base]++;
        if (!((plan.oom_lane_mask >> lane) & 1) || ++n_starts != plan.oom_at_start) return ZK_OK;
        oom = true;
        return fail(ZK_ERR_OUT_OF_MEMORY, "workspaces do not fit");
    }
    zk_status ready(const Job& j, int) {
        step();
        return (int)j.index_base == plan.bad_job ? fail(ZK_ERR_INVALID_ARGUMENT, "statement " + std::to_string(j.index_base)) : ZK_OK;
    }
    zk_status prove(const Job& j, int) {
        step();
        rec.proved[j.index_base]++;
        rec.proved_by_lane[lane]++;
        if (oom) g_ahead_oom++;   // the start that ran out of memory was the NEXT job's: this one is proved all the same
        return ZK_OK;
    }
    void drain_device() { rec.drained[lane]++; }
    void release() { rec.released[lane]++; }
    std::string message() const { return msg; }
};

// The host witness engine as a lane: ONE helper thread (the SlotThread ChunkWitness uses, driven as ChunkWitness drives it)
// makes the witnesses of a slot.  What the lane loop's order - start(next) before ready(current) - must leave intact: the
// current job's witnesses are there when ready() returns, and the next job's are still the helper's business, not waited
// for, when prove() of the current one begins.
struct HostFakeLane : FakeLane {
    zkpipe::SlotThread helper;
    int last_started_slot = -1;
    zk_status start(const Job& j, int slot) {
        helper.join();
        rec.started[j.index_base]++;
        last_started_slot = slot;
        const size_t job = j.index_base;
        const uint64_t us = 100 + (rng >> 40) % 200;
        Record* r = &rec;
        helper.start(slot, [r, job, us] {
            std::this_thread::sleep_for(std::chrono::microseconds(us));
            r->wit_done[job] = 1;
        });
        return ZK_OK;
    }
    zk_status ready(const Job& j, int slot) {
        helper.join_slot(slot);
        if (!rec.wit_done[j.index_base]) rec.not_ready++;
        return (int)j.index_base == plan.bad_job ? fail(ZK_ERR_INVALID_ARGUMENT, "statement " + std::to_string(j.index_base)) : ZK_OK;
    }
    zk_status prove(const Job& j, int slot) {
        if (last_started_slot != slot) (helper.live == (slot ^ 1) ? rec.beside : rec.not_beside)++;   // (a next job was started this turn)
        return FakeLane::prove(j, slot);
    }
    void drain_device() {
        helper.join();
        FakeLane::drain_device();
    }
};

// a pipeline of fake lanes; jobs are numbered through index_base
struct Pipe {
    LaneQueue Q;
    Record rec;
    Plan plan;
    std::vector<std::thread> threads;
    int next_job = 0;
    Pipe(int lanes, uint64_t seed, const Plan& p) : plan(p) {
        Q.open(lanes);
        for (int l = 0; l < lanes; l++)
            threads.emplace_back([this, l, seed] {
                if (plan.host) {
                    HostFakeLane lane{{rec, plan, l, seed * 1000003 + l}};
                    zkpipe::lane_run(Q, l, lane);
                } else {
                    FakeLane lane{rec, plan, l, seed * 1000003 + l};
                    zkpipe::lane_run(Q, l, lane);
                }
            });
    }
    void submit(int n) {
        std::vector<Job> jobs;
        for (int i = 0; i < n; i++) jobs.push_back(Job{nullptr, nullptr, nullptr, 1, (size_t)next_job++});
        Q.submit(jobs.data(), jobs.size());
    }
    zk_status wait(std::string* msg = nullptr) {
        std::string m;
        const zk_status rc = Q.wait(&m);
        if (msg) *msg = m;
        return rc;
    }
    void close() {
        Q.close();
        for (auto& t : threads) t.join();
        threads.clear();
    }
    ~Pipe() {
        if (!threads.empty()) close();
    }
    bool each_proved_once(int first, int last) const {
        for (int j = first; j < last; j++)
            if (rec.proved[j] != 1) return false;
        return true;
    }
};

void plain_stream(int lanes, uint64_t seed, bool wait_between) {
    Pipe P(lanes, seed, Plan{});
    for (int n : {1, 5, 2}) {
        P.submit(n);
        if (wait_between) CHECK(P.wait() == ZK_OK, "lanes %d seed %d", lanes, (int)seed);
    }
    CHECK(P.wait() == ZK_OK, "lanes %d seed %d", lanes, (int)seed);
    CHECK(P.each_proved_once(0, 8), "lanes %d seed %d", lanes, (int)seed);
    CHECK(P.Q.lanes() == lanes, "lanes %d", lanes);
    P.close();
}

// lanes beyond the first (mask) run out of memory at their first start / at their second, the start of the job taken ahead
// when there was one: each retires, having proved at_start - 1 jobs, and every job is proved once by the lanes that are left
void oom_retires(int lanes, uint64_t seed, int mask, int at_start) {
    Plan plan;
    plan.oom_lane_mask = mask;
    plan.oom_at_start = at_start;
    Pipe P(lanes, seed, plan);
    int left = lanes;
    for (int l = 1; l < lanes; l++) left -= (mask >> l) & 1;
    for (int k = 0; k < MAX_ROUNDS && (k == 0 || P.Q.lanes() > left); k++) {
        P.submit(12);
        CHECK(P.wait() == ZK_OK, "mask %d at %d seed %d", mask, at_start, (int)seed);
    }
    CHECK(P.Q.lanes() == left, "lanes %d, expected %d", P.Q.lanes(), left);
    P.submit(3);   // the survivors go on
    CHECK(P.wait() == ZK_OK, "after the retirement");
    CHECK(P.each_proved_once(0, P.next_job), "mask %d at %d seed %d", mask, at_start, (int)seed);
    for (int l = 0; l < lanes; l++) {
        const int retired = l > 0 && ((mask >> l) & 1);
        CHECK(P.rec.released[l] == retired && P.rec.drained[l] == retired, "lane %d released %d", l, (int)P.rec.released[l]);
        if (retired) CHECK(P.rec.proved_by_lane[l] == at_start - 1, "lane %d proved %d", l, (int)P.rec.proved_by_lane[l]);
    }
    P.close();
}

// every lane beyond the first retires at its first start while lane 0 works: one lane is left
void all_retire_at_once(uint64_t seed) { oom_retires(4, seed, 0xe, 1); }

// lane 0 out of memory is a failure of the stream, not a retirement
void lane0_oom_fails(int lanes, uint64_t seed) {
    Plan plan;
    plan.oom_lane_mask = 1;
    Pipe P(lanes, seed, plan);
    std::string msg;
    zk_status rc = ZK_OK;
    for (int k = 0; k < MAX_ROUNDS && rc == ZK_OK; k++) {   // (until lane 0 has taken a job)
        P.submit(6);
        rc = P.wait(&msg);
    }
    CHECK(rc == ZK_ERR_OUT_OF_MEMORY && msg == "workspaces do not fit", "lanes %d seed %d: %s", lanes, (int)seed, msg.c_str());
    CHECK(P.Q.lanes() == lanes && P.rec.released[0] == 0, "lane 0 retired");
    for (int j = 0; j < P.next_job; j++) CHECK(P.rec.proved[j] <= 1, "job %d proved %d times", j, (int)P.rec.proved[j]);
    P.submit(2);   // (its second start is no fault)
    CHECK(P.wait() == ZK_OK && P.each_proved_once(P.next_job - 2, P.next_job), "lanes %d seed %d: the stream after a failure", lanes, (int)seed);
    P.close();
}

// a malformed statement: the first error wins, what is behind it drains without work, wait() reports once, the stream goes on
void failing_job(int lanes, uint64_t seed) {
    Plan plan;
    plan.bad_job = 2;
    Pipe P(lanes, seed, plan);
    P.submit(40);
    std::string msg;
    CHECK(P.wait(&msg) == ZK_ERR_INVALID_ARGUMENT && msg == "statement 2", "lanes %d seed %d: %s", lanes, (int)seed, msg.c_str());
    CHECK(P.rec.proved[2] == 0, "the failing job was proved");
    for (int j = 0; j < 40; j++)
        CHECK(P.rec.proved[j] <= 1 && P.rec.started[j] <= 1, "job %d: %d starts, %d proofs", j, (int)P.rec.started[j], (int)P.rec.proved[j]);
    // one lane: job 3 was taken ahead and started before job 2 failed; everything behind it drains with no fake called
    if (lanes == 1)
        for (int j = 3; j < 40; j++) CHECK(P.rec.started[j] == (j == 3) && P.rec.proved[j] == 0, "job %d was worked on behind the failure", j);
    CHECK(P.wait() == ZK_OK, "the failure was reported twice");
    P.plan.bad_job = -1;   // (the lanes are idle: everything submitted is over)
    P.submit(4);
    CHECK(P.wait() == ZK_OK && P.each_proved_once(40, 44), "lanes %d seed %d: the stream after a failure", lanes, (int)seed);
    P.close();
}

// jobs submitted behind a failure that wait() has not reported yet drain without a fake being called, however they are taken
void drains_behind_a_failure(uint64_t seed) {
    Plan plan;
    plan.bad_job = 0;
    Pipe P(1, seed, plan);
    P.submit(1);
    while (P.rec.drained[0] == 0) std::this_thread::yield();   // (the job has failed: the lane drains its device before it says so)
    P.submit(3);
    std::string msg;
    CHECK(P.wait(&msg) == ZK_ERR_INVALID_ARGUMENT && msg == "statement 0", "seed %d: %s", (int)seed, msg.c_str());
    for (int j = 0; j < 4; j++) CHECK(P.rec.started[j] == (j == 0) && P.rec.proved[j] == 0, "job %d was worked on behind the failure", j);
    P.close();
}

// the host engine, lane 0 alone: ten jobs in one submit, so every turn but the last starts a next job
void host_engine_overlaps(uint64_t seed) {
    Plan plan;
    plan.host = true;
    Pipe P(1, seed, plan);
    P.submit(10);
    CHECK(P.wait() == ZK_OK && P.each_proved_once(0, 10), "seed %d", (int)seed);
    CHECK(P.rec.not_ready == 0, "seed %d: ready() returned before the witnesses were there, %d times", (int)seed, (int)P.rec.not_ready);
    CHECK(P.rec.beside == 9 && P.rec.not_beside == 0, "seed %d: the next job's witnesses ran beside the proof %d times, were waited for %d times",
          (int)seed, (int)P.rec.beside, (int)P.rec.not_beside);
    P.close();
}

// ... and a failing job: the helper thread of the job started behind it is over before wait() returns (it reads the caller's
// statements), the rest drains, the stream goes on
void host_engine_failing_job(uint64_t seed) {
    Plan plan;
    plan.host = true;
    plan.bad_job = 2;
    Pipe P(1, seed, plan);
    P.submit(8);
    std::string msg;
    CHECK(P.wait(&msg) == ZK_ERR_INVALID_ARGUMENT && msg == "statement 2", "seed %d: %s", (int)seed, msg.c_str());
    CHECK(P.rec.started[3] == 1 && P.rec.wit_done[3] == 1, "seed %d: a helper thread outlived wait()", (int)seed);
    for (int j = 2; j < 8; j++) CHECK(P.rec.proved[j] == 0 && P.rec.started[j] == (j <= 3), "job %d was worked on behind the failure", j);
    P.plan.bad_job = -1;
    P.submit(3);
    CHECK(P.wait() == ZK_OK && P.each_proved_once(8, 11) && P.rec.not_ready == 0, "seed %d: the stream after a failure", (int)seed);
    P.close();
}

// a lane that never got its context reports that and drains what it finds
void lane_without_context(int lanes, int which, uint64_t seed) {
    Plan plan;
    plan.no_context_lane = which;
    Pipe P(lanes, seed, plan);
    std::string msg;
    zk_status rc = ZK_OK;
    for (int k = 0; k < MAX_ROUNDS && rc == ZK_OK; k++) {   // (with other lanes alive a wait() can be over before the lane has reported)
        P.submit(6);
        rc = P.wait(&msg);
    }
    CHECK(rc == ZK_ERR_DEVICE && msg == "no context", "lanes %d seed %d", lanes, (int)seed);
    for (int j = 0; j < P.next_job; j++) CHECK(P.rec.proved[j] <= 1, "job %d proved %d times", j, (int)P.rec.proved[j]);
    CHECK(P.rec.proved_by_lane[which] == 0, "a lane without a context proved");
    P.close();
}

void close_idle(int lanes) {
    Pipe P(lanes, 1, Plan{});
    P.close();
}

void close_after_failing_submit(int lanes, uint64_t seed) {
    Plan plan;
    plan.bad_job = 0;
    Pipe P(lanes, seed, plan);
    P.submit(5);
    P.close();   // waits for the five, reports nothing
    for (int j = 0; j < 5; j++) CHECK(P.rec.proved[j] <= 1, "job %d proved %d times", j, (int)P.rec.proved[j]);
    CHECK(P.rec.proved[0] == 0, "the failing job was proved");
}

}  // namespace

int main() {
    for (uint64_t seed = 1; seed <= 5; seed++) {
        for (int lanes : {1, 2, 4}) {
            plain_stream(lanes, seed, true);
            plain_stream(lanes, seed, false);
            lane0_oom_fails(lanes, seed);
            failing_job(lanes, seed);
            close_after_failing_submit(lanes, seed);
        }
        oom_retires(2, seed, 0x2, 1);
        oom_retires(3, seed, 0x4, 1);
        oom_retires(2, seed, 0x2, 2);
        oom_retires(4, seed, 0xa, 2);
        all_retire_at_once(seed);
        drains_behind_a_failure(seed);
        host_engine_overlaps(seed);
        host_engine_failing_job(seed);
        lane_without_context(1, 0, seed);
        lane_without_context(2, 1, seed);
        lane_without_context(3, 0, seed);
    }
    for (int lanes : {1, 2, 4}) close_idle(lanes);
    CHECK(g_ahead_oom > 0, "no lane ever ran out of memory at the start of a job taken ahead");
    if (g_failures) {
        fprintf(stderr, "%d checks failed\n", g_failures);
        return 1;
    }
    printf("pipeline lanes: all scenarios held\n");
    return 0;
}
