// ---------------------------------------------------------------------------------------------------------------------
// The flag hand-overs of the persistent GRU phase: the protocol, once.  Included by dfx_nn_kernels.h; the parties are the recurrences
// (dfx_gru_h3_run, dfx_gru_p2_run), their followers (dfx_k_emb_follow, dfx_k_proj_follow, dfx_k_proj_follow_x32), the producer kernels that
// announce themselves (dfx_publish) and the flag kernels at the end of this file.  The host side of the same words is DfxSyncLayout (dfx_model.hip).
//
// FLAGS.  Every flag is one 32-bit word that only grows over the life of the model (no resets): a base the host advances per pass plus a count of
// chunks (base + k + 1) or of steps (pbase + steps).  A waiter compares `flag - want` as a SIGNED difference, so wrap-around is harmless and a word
// left over from an earlier pass reads as "not yet".
//
// WHO RAISES AND WHO POLLS WHAT.  The time axis is cut into K chunks.  Chunk level: `ready` (one word per layer) says that the layer's input
// projection of a chunk exists — raised by the projection kernel's last workgroup (dfx_publish) or by dfx_k_flag_set behind it on its stream, polled
// by the layer's recurrences unless a follower feeds them; `done[group]` says that a recurrence has completed a chunk of y — raised by the recurrence,
// polled by dfx_k_wait_ge in front of the host-launched consumers.  Block level, per 16-clip group, counting steps: `yprog` is raised by a recurrence
// every `yblk` steps (and at the end of the sequence) and polled by the follower of the layer above (or the emb follower, whose own word `embprog`
// the first decoder layers' projection followers poll); `giprog` is raised by a projection follower per block of its gi rows and polled by its
// layer's recurrence one step before it requests the block's first row.  Pair form: half p of a pair raises its step flag `pflag` every step and
// polls the partner's; towards the words above it stands for group 2 pg + p and polls the giprog of both groups.
//
// THE SAME-XCD RULE.  A producer and a consumer that share an L2 need neither the L2 write-back of an agent-scope release nor the L2 invalidate of an
// agent-scope acquire — the invalidate alone throws the XCD's share of the streamed W_hh out of the L2 every 16 steps of every recurrence on it
// (measured with both left out: 7.9 -> 7.3 us per step).  Workgroups go round-robin over the XCDs with a rotation that differs per launch, so every
// party REGISTERS the XCD it runs on: its registration word is tag | (xcd + 1), the tag (low four bits zero) unique per pass.  A hand-over whose
// partner's word equals the own one is LIGHT: every wave drains its stores (DFX_VMEM_DRAIN) in front of a barrier, thread 0 raises the flag with a
// relaxed store, and the consumer, behind the barrier that follows its poll, invalidates its L1 only (DFX_L1_INV).  Anything else — partner
// elsewhere, or not registered yet — takes the full form: release store, agent-scope acquire fence.  A polled line stays in the L1 and DFX_L1_INV
// does not drop it: the light form is right because every line it protects is FIRST TOUCHED AFTER ITS FLAG has been seen — nobody reads a row of a
// block ahead of the block's flag.
//
// TIMEOUTS.  Every wait is bounded: `spin_limit` polls (DFX_SYNC_SPIN_LIMIT, ~2 s with the sleeps below).  A wait that runs out raises err[2] — the
// pass is reported as failed and its output poisoned, never hidden — and latches the workgroup's waiter `dead`: that workgroup waits for nothing more
// and runs to its end on whatever it finds, so that a starved party holds the device for one limit, not for one per block.
// ---------------------------------------------------------------------------------------------------------------------
#pragma once

#define DFX_SYNC_SPIN_LIMIT (1 << 22)   /* default bound of every flag wait: polls with s_sleep, ~2 s (dfx_model::spin_limit, DFX_SYNC_SPIN_LIMIT) */

// the registration word of the calling workgroup under a pass's tag / "is *word mine": its owner runs on this XCD and has registered in this pass
static __device__ __forceinline__ unsigned int dfx_sync_my_word(unsigned int tag) { return tag | (unsigned int)(dfx_xcc_id() + 1); }
static __device__ __forceinline__ bool dfx_sync_is_mine(const unsigned int *word, unsigned int tag) {
    return __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == dfx_sync_my_word(tag);
}

// The waits of one workgroup, held by its thread 0.  SLEEP is s_sleep's immediate between two polls, 0 = none.
struct DfxWaiter {
    int spin_limit;      // polls before a wait gives up
    unsigned int *err;   // err[2] is raised by a wait that gave up
    bool dead = false;   // a wait of this workgroup has timed out: no further wait holds the device

    template <int SLEEP>
    __device__ __forceinline__ void wait_ge(const unsigned int *flag, unsigned int want) {
        int spins = 0;
        while (!dead && (int)(__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - want) < 0) {
            if (++spins > spin_limit) {
                dfx_raise(err + 2);
                dead = true;
                break;
            }
            if constexpr (SLEEP > 0) __builtin_amdgcn_s_sleep(SLEEP);
        }
    }
    // until *word is a registration of this pass (any XCD); returns the word it read last
    template <int SLEEP>
    __device__ __forceinline__ unsigned int wait_registered(const unsigned int *word, unsigned int tag) {
        unsigned int v = 0u;
        int spins = 0;
        while (!dead && (((v = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & ~15u) != tag || (v & 15u) == 0u)) {
            if (++spins > spin_limit) {
                dfx_raise(err + 2);
                dead = true;
                break;
            }
            if constexpr (SLEEP > 0) __builtin_amdgcn_s_sleep(SLEEP);
        }
        return v;
    }
};

// the producer's side of a hand-over: thread 0, behind a barrier in front of which EVERY wave has drained its stores (light) / whose workgroup's
// stores the release covers (full)
static __device__ __forceinline__ void dfx_sync_raise(unsigned int *flag, unsigned int value, bool light) {
    if (light) __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
// the consumer's side, behind the barrier that follows the poll (every thread)
static __device__ __forceinline__ void dfx_sync_acquire(bool light) {
    if (light) DFX_L1_INV();
    else __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// The registration words of one party of the phase's followers and one-CU recurrences (the pair form keeps its words in DfxGpSync).
struct DfxXcd {
    unsigned int *me = nullptr;            // this party's registration word: tag | (xcd + 1)
    const unsigned int *prod = nullptr;    // the registration word of the party whose output this one consumes, or null
    const unsigned int *cons = nullptr;    // ... of the party that consumes this one's output, or null
    const unsigned int *cons2 = nullptr;   // a second consumer (the emb follower feeds two projection followers), or null
    unsigned int tag = 0;                  // of this pass (low four bits zero)
    unsigned int *stat = nullptr;          // dev aid: counts light releases
};
static __device__ __forceinline__ void dfx_xcd_register(const DfxXcd &X) {
    if (X.me && threadIdx.x == 0) __hip_atomic_store(X.me, dfx_sync_my_word(X.tag), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
static __device__ __forceinline__ bool dfx_xcd_same(const DfxXcd &X, const unsigned int *other) { return other && dfx_sync_is_mine(other, X.tag); }
static __device__ __forceinline__ void dfx_xcd_acquire(const DfxXcd &X) { dfx_sync_acquire(dfx_xcd_same(X, X.prod)); }
static __device__ __forceinline__ void dfx_xcd_release(const DfxXcd &X, unsigned int *flag, unsigned int value) {
    const bool light = dfx_xcd_same(X, X.cons) && (!X.cons2 || dfx_xcd_same(X, X.cons2));
    dfx_sync_raise(flag, value, light);
    if (light && X.stat) __hip_atomic_fetch_add(X.stat, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// A follower workgroup picks the 16-clip group it serves: one whose RECURRENCE runs on this workgroup's XCD (workgroups go round-robin over the 8
// XCDs with a rotation that differs from launch to launch, so block index g of the follower launch is usually NOT next to group g's recurrence).
// rec[g] = registration words of the recurrences of one layer (all layers of a launch share the mapping), claim[8] = slots handed out per XCD
// (zeroed by the host before the launch).  Own XCD first, then the others in turn: as many workgroups as groups, so everyone finds exactly one —
// also if the dispatch was not an exact round robin.  Thread 0 decides, the result travels through *slot (LDS).  rec == nullptr: group = fallback.
static __device__ __forceinline__ int dfx_xcd_claim(const unsigned int *rec, unsigned int tag, int groups, unsigned int *claim, int fallback, DfxWaiter &W, int *slot) {
    if (!rec || groups > 64) return fallback;
    if (threadIdx.x == 0) {
        auto xcd_of = [&](int g) { return (int)(__hip_atomic_load(rec + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 15u) - 1; };   // (re-read: no array in scratch)
        for (int g = 0; g < groups; ++g) W.wait_registered<4>(rec + g, tag);   // every recurrence of this pass has registered (they start first)
        int got = -1;
        const int x0 = dfx_xcc_id();
        for (int d = 0; d < 8 && got < 0 && !W.dead; ++d) {
            const int x = (x0 + d) & 7;
            int cnt = 0;
            for (int g = 0; g < groups; ++g) cnt += xcd_of(g) == x;
            if (!cnt) continue;
            const unsigned int k = __hip_atomic_fetch_add(claim + x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((int)k >= cnt) continue;
            for (int g = 0, j = 0; g < groups; ++g)
                if (xcd_of(g) == x && j++ == (int)k) got = g;
        }
        *slot = got < 0 ? fallback : got;   // (got < 0: registrations timed out; err is raised)
    }
    __syncthreads();
    const int r = *slot;
    __syncthreads();
    return r;
}

// A producer kernel of the persistent GRU phase announces its own completion (round 5): every workgroup, when its rows are stored, adds itself to a
// counter; the last one resets the counter and raises the flag the consumers poll — the dfx_k_flag_set launch behind the producer (and the ~8 us of
// host enqueue and dispatch it costs per layer and chunk) is gone.  cnt == nullptr: nothing (every launch outside that phase).
struct DfxPublish {
    unsigned int *cnt = nullptr;   // completion counter of this producer (one word per stream: launches on a stream do not overlap)
    unsigned int *flag = nullptr;
    unsigned int value = 0, nblocks = 0;
};
static __device__ __forceinline__ void dfx_publish(const DfxPublish &P) {
    if (!P.cnt) return;
    DFX_VMEM_DRAIN();  // (s_barrier does not wait for the other waves' stores: each wave drains its own in front of it)
    __syncthreads();   // the workgroup's stores happen before thread 0's release below (one L2 write-back per workgroup; a release fence in
                       // every thread in front of the barrier is one per WAVE and costs the step 1.6 ms, measurements R5.10)
    if (threadIdx.x == 0) {
        const unsigned int old = __hip_atomic_fetch_add(P.cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (old + 1u == P.nblocks) {
            __hip_atomic_store(P.cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(P.flag, P.value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// flag kernels of the persistent GRU phase: dfx_k_flag_set runs behind a producer on its stream (the kernel boundary in front of it
// has made the producer's writes visible), dfx_k_wait_ge holds its stream until all n flags have reached the target
__global__ void dfx_k_flag_set(unsigned int *flag, unsigned int value) {
    if (threadIdx.x == 0) __hip_atomic_store(flag, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ void dfx_k_wait_ge(const unsigned int *flags, int n, unsigned int target, unsigned int *err, int spin_limit) {
    bool ok = false;
    int spins = 0;
    while (!ok) {
        ok = true;
        for (int i = threadIdx.x; i < n; i += blockDim.x)
            ok = ok && (int)(__hip_atomic_load(flags + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) >= 0;
        ok = __all(ok);   // one wave
        if (!ok) {
            if (++spins > spin_limit) {
                if (threadIdx.x == 0) dfx_raise(err + 2);
                break;
            }
            __builtin_amdgcn_s_sleep(16);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// Handshake of dfx_model_create (DFX_Q_HWQ_PROBE): one single-wave launch per stream of the persistent phase; each adds itself to a
// counter and waits, bounded, until all n have arrived — which only happens if the n streams really run at the same time (streams
// that share a hardware queue run one after the other: the first then waits in vain and raises *fail).
__global__ void dfx_k_probe_meet(unsigned int *cnt, unsigned int n, int spin_limit, unsigned int *fail) {
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int spins = 0;
        while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < n) {
            if (++spins > spin_limit) {
                dfx_raise(fail);
                break;
            }
            __builtin_amdgcn_s_sleep(16);
        }
    }
}
