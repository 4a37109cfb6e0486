// libzkamd, the lanes of a zk_pipeline: the queue of chunk jobs its worker threads share, the loop each of them runs, and the
// helper thread of the host witness engine (statement_route.h ChunkWitness) that such a loop drives.
// Nothing here touches the GPU - a lane's device work comes in as the Lane parameter of lane_run, and the message of a
// failing step comes from it - so the interleavings of several lanes, of retirement and of a failed stream are exercised on
// the CPU (tests/pipeline_lanes_main.cpp, under ThreadSanitizer).  Part of zkamd.cpp's translation unit.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include "../../include/zkamd.h"

namespace zkpipe {

// one chunk of a submit: n statements, their (r, s) and where their proofs go; index_base: the place of st[0] in its submit
struct Job {
    const zk_transfer_statement* st;
    const uint8_t* rs;
    uint8_t* out;
    size_t n, index_base;
};

// One helper thread over two slots: it works on one slot at a time, and whoever asks for a slot waits for the thread only if
// that slot is the one it is working on - so a caller may start slot B and then ask for slot A without waiting for B.
// fn must not throw.
struct SlotThread {
    std::thread t;
    int live = -1;   // the slot the thread was started for and has not been joined since
    template <class Fn>
    void start(int slot, Fn fn) {
        join();
        t = std::thread(std::move(fn));
        live = slot;
    }
    void join_slot(int slot) {
        if (live == slot) join();
    }
    void join() {
        if (t.joinable()) t.join();
        live = -1;
    }
    ~SlotThread() { join(); }
};

// Everything the lanes and the callers of a pipeline share, behind one lock.  A job is IN FLIGHT from submit() until exactly
// one lane counts it: done() after it was proved, failed or drained, or retire() for the one a leaving lane had proved.
class LaneQueue {
    mutable std::mutex mu;
    std::condition_variable cv;
    std::deque<Job> q;
    size_t in_flight = 0;
    int live_lanes = 1;        // lanes started, minus the ones that retired
    zk_status err = ZK_OK;     // the first failure since the last wait(), with its text
    std::string err_msg;
    bool stop = false;

    void fail_with(zk_status st, const std::string& msg) {   // mu held
        if (err != ZK_OK) return;
        err = st;
        err_msg = msg;
    }

public:
    enum Taken { STOP, WORK, DRAIN };   // DRAIN: the stream has failed - the job is counted done without work

    void open(int lanes) { live_lanes = lanes; }   // before the lanes start
    int lanes() const {
        std::lock_guard<std::mutex> lk(mu);
        return live_lanes;
    }
    void submit(const Job* jobs, size_t n) {
        std::lock_guard<std::mutex> lk(mu);
        q.insert(q.end(), jobs, jobs + n);
        in_flight += n;
        cv.notify_all();
    }
    // the next job, waiting for one
    Taken take(Job* j) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || !q.empty(); });
        if (stop) return STOP;
        *j = q.front();
        q.pop_front();
        return err != ZK_OK ? DRAIN : WORK;
    }
    // the job behind the current one, if there is one now - and, with several lanes, only if the other lanes still find one each;
    // failed: whether the stream has failed by now
    bool take_ahead(Job* j, bool* failed) {
        std::lock_guard<std::mutex> lk(mu);
        *failed = err != ZK_OK;
        if (q.size() < (size_t)live_lanes) return false;
        *j = q.front();
        q.pop_front();
        return true;
    }
    // one job is over; st != ZK_OK: it failed (the first failure of the stream is the one wait() reports)
    void done(zk_status st, const std::string& msg) {
        std::lock_guard<std::mutex> lk(mu);
        if (st != ZK_OK) fail_with(st, msg);
        in_flight--;
        cv.notify_all();
    }
    // A lane leaves: the job it took ahead (null: none) and its current one go back to the head of the queue in their
    // order - unless the current one was proved, which is counted here.  release() frees what the lane holds, outside the
    // lock and before the other lanes are woken for the jobs.
    template <class Release>
    void retire(const Job& cur, bool cur_proved, const Job* ahead, Release&& release) {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (ahead) q.push_front(*ahead);
            if (cur_proved) in_flight--;
            else q.push_front(cur);
            live_lanes--;
        }
        release();
        std::lock_guard<std::mutex> lk(mu);
        cv.notify_all();
    }
    // a lane that never got its context: reports that once and counts the jobs it finds done, so that wait() and close()
    // never block on jobs nobody will take
    void drain_without_context(zk_status st, const std::string& msg) {
        std::unique_lock<std::mutex> lk(mu);
        fail_with(st, msg);
        for (;;) {
            cv.wait(lk, [&] { return stop || !q.empty(); });
            if (stop) return;
            q.pop_front();
            in_flight--;
            cv.notify_all();
        }
    }
    // everything submitted so far is over: the first failure among it, reported once - the stream is usable again
    zk_status wait(std::string* msg) {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return in_flight == 0; });
        const zk_status rc = err;
        if (rc != ZK_OK) *msg = err_msg;
        err = ZK_OK;
        err_msg.clear();
        return rc;
    }
    // ... and the lanes return from take()
    void close() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return in_flight == 0; });
        stop = true;
        cv.notify_all();
    }
};

// The worker of lane `lane`.  What a lane can do, each step a status (message(): the text of the last one that failed):
//   open()              its context (whatever status it fails with, the stream reports ZK_ERR_DEVICE with the lane's message)
//   start(job, slot)    begin the witnesses of a job in one of two slots
//   ready(job, slot)    ... they are there
//   prove(job, slot)    the proofs of the job, written when it returns
//   drain_device()      nothing of this lane is in flight any more, on the device or in a helper thread
//   release()           give up its workspaces (a lane beyond the first, as it retires)
// The witnesses of the job behind the current one are STARTED before the current one's are awaited and proved, so they run
// beside its proving.  A lane beyond the first that runs out of memory retires: its workspaces are allocated when it proves
// its first chunk, the lane count was only a hint, and the pipeline degrades to fewer lanes instead of failing in the
// middle of a batch.  Lane 0 never retires: its failure is the stream's.
template <class Lane>
void lane_run(LaneQueue& Q, int lane, Lane& L) {
    if (L.open() != ZK_OK) return Q.drain_without_context(ZK_ERR_DEVICE, L.message());
    Job cur{}, nxt{};
    bool have_cur = false;   // (the job taken ahead in the turn before, its witnesses started)
    for (int slot = 0;; slot ^= 1) {
        zk_status rc = ZK_OK, rc_next = ZK_OK;
        if (!have_cur) {
            const LaneQueue::Taken t = Q.take(&cur);
            if (t == LaneQueue::STOP) return;
            if (t == LaneQueue::WORK) rc = L.start(cur, slot);
        }
        bool failed;
        const bool have_nxt = Q.take_ahead(&nxt, &failed);
        const bool work = !failed;   // a failed stream drains without doing work
        if (have_nxt && work && rc == ZK_OK) rc_next = L.start(nxt, slot ^ 1);
        if (work && rc == ZK_OK) rc = L.ready(cur, slot);
        if (work && rc == ZK_OK) rc = L.prove(cur, slot);
        const std::string msg = rc != ZK_OK || rc_next != ZK_OK ? L.message() : std::string();
        // nothing of a failed job stays in flight when wait() returns: the device is drained BEFORE the job is counted done
        if (rc != ZK_OK || rc_next != ZK_OK) L.drain_device();
        if (lane > 0 && (rc == ZK_ERR_OUT_OF_MEMORY || rc_next == ZK_ERR_OUT_OF_MEMORY))
            // (when starting the NEXT job is what ran out of memory, the current one is proved and counted)
            return Q.retire(cur, work && rc == ZK_OK, have_nxt ? &nxt : nullptr, [&] { L.release(); });
        Q.done(rc != ZK_OK ? rc : rc_next, msg);
        cur = nxt;
        have_cur = have_nxt;
    }
}

}  // namespace zkpipe
