// stage.h — the host staging ring behind impala_stage* / impala_slot_* (include/impala_hip.h):
// device batch slots filled by H2D copies while the previous batch's step runs.  Included by
// impala.hip after its error helpers (fail, CK, CK_LAUNCH) and kernels.h; the extern "C" entry
// points there check their arguments and forward to the functions here, which take the ring,
// not the learner handle.
//
// The copy path: obs by hipMemcpyAsync (SDMA) in two halves on two copy streams, the four small
// fields in one small pull launch (h2d_pull_kernel) when the host batch is page-locked and
// device-mapped, else four more SDMA copies.  Beside the fp32 step (profiles/r04hs: H2D
// bandwidth A/B) SDMA on 1 / 2 / 4 streams kept 41-43 / 46.4 / 43.9 GB/s, while the pull kernel
// for the whole batch (8 x 256 threads, 45-48 GB/s alone and the round-1 default) fell to
// 36 GB/s and slowed the trunk forward it shares CUs with from 63 to 190-210 us (rocprofv3
// kernel trace, r04hs).  That path, the stream-count override and the per-row SDMA form of row
// staging (0.58-0.68 ms per step) have been removed.
#pragma once

namespace {

constexpr int kCopyStreams = 2;

// The copy streams, one reference-counted pair per device shared by every ring on it: a
// process's streams share GPU_MAX_HW_QUEUES (4) hardware queues, and each handle's own pair of
// copy streams took a share of them (a second handle's staging ran at 0.42 instead of 0.30 ms
// per step beside the first's, profiles/r06w).  The last ring's release destroys them.
struct SharedH2D {
  int device = -1, refs = 0;
  hipStream_t s[kCopyStreams] = {};
};
std::mutex g_h2d_mu;
SharedH2D g_h2d[16];

struct StageRing {
  // `ready` = the slot's copies are done, `done` = the steps that read it are done
  struct Slot {
    char* mem = nullptr;
    impala_batch dev{};
    hipEvent_t ready = nullptr, done = nullptr;
    // impala_stage_rows: the slot's page-locked host block (the same layout), allocated at the
    // first row staging into the slot
    char* host_blk = nullptr;
  };
  static constexpr int kMaxSlots = 8;
  Slot slots[kMaxSlots];
  int n_slots = 0;
  int device = 0;
  bool ppo = false;  // PPO handles: no discounts field
  impala_host::StageLayout lay;
  // h2d[0] carries the small fields and the first half of obs, joins h2d[1] (the second half)
  // through `join` and signals `ready`; null until the first stage_init
  hipStream_t h2d[kCopyStreams] = {};
  hipEvent_t join = nullptr;
  bool small_pull = true;  // the four small fields in one pull launch (else SDMA copies)
  impala_host::HostPool* pool = nullptr;   // impala_stage_rows' collate (lazily started)
  impala_host::Stager* stager = nullptr;   // impala_stage_rows_async's thread (lazily started)
};
static_assert(StageRing::kMaxSlots == impala_host::Stager::kSlots, "one job counter per slot");

int acquire_h2d(StageRing& r) {
  std::lock_guard<std::mutex> lk(g_h2d_mu);
  SharedH2D* e = nullptr;
  for (auto& x : g_h2d)
    if (x.refs > 0 && x.device == r.device) e = &x;
  if (!e) {
    for (auto& x : g_h2d)
      if (x.refs == 0) {
        e = &x;
        break;
      }
    if (!e) return fail(IMPALA_E_STATE, "impala_stage_init: too many staging stream sets");
    for (int i = 0; i < kCopyStreams; ++i) {
      if (hipStreamCreateWithFlags(&e->s[i], hipStreamNonBlocking) != hipSuccess) {
        for (int j = 0; j < i; ++j) (void)hipStreamDestroy(e->s[j]);
        return fail(IMPALA_E_STATE, "impala_stage_init: hipStreamCreate failed");
      }
    }
    e->device = r.device;
  }
  ++e->refs;
  for (int i = 0; i < kCopyStreams; ++i) r.h2d[i] = e->s[i];
  return 0;
}

void release_h2d(StageRing& r) {
  if (!r.h2d[0]) return;
  std::lock_guard<std::mutex> lk(g_h2d_mu);
  for (auto& x : g_h2d)
    if (x.refs > 0 && x.device == r.device && x.s[0] == r.h2d[0]) {
      if (--x.refs == 0) {
        for (auto s : x.s) (void)hipStreamDestroy(s);
        x = SharedH2D{};
      }
      break;
    }
  for (auto& s : r.h2d) s = nullptr;
}

// the staging jobs of `slot` (every slot when < 0) queued by impala_stage_rows_async have run;
// a failed one's status is returned here
int wait_staged(StageRing& r, int slot) {
  if (!r.stager) return 0;
  std::string m;
  if (int st = r.stager->wait(slot, m)) return fail(st, "impala_stage_rows_async: " + m);
  return 0;
}

// free the slots (the copy streams, pool and staging thread stay for the next stage_init)
void free_slots(StageRing& r) {
  if (r.stager) {  // no staging job may still be writing into the ring
    std::string m;
    (void)r.stager->wait(-1, m);
  }
  for (auto s : r.h2d)
    if (s) (void)hipStreamSynchronize(s);
  for (auto& s : r.slots) {
    if (s.done) (void)hipEventSynchronize(s.done);
    if (s.ready) (void)hipEventDestroy(s.ready);
    if (s.done) (void)hipEventDestroy(s.done);
    if (s.mem) (void)hipFree(s.mem);
    if (s.host_blk) (void)hipHostFree(s.host_blk);
    s = StageRing::Slot{};
  }
  r.n_slots = 0;
}

// impala_destroy: everything the ring owns
void stage_destroy(StageRing& r) {
  free_slots(r);
  release_h2d(r);
  if (r.join) (void)hipEventDestroy(r.join);
  delete r.stager;  // (free_slots already waited for its jobs)
  delete r.pool;
  r = StageRing{};
}

// Where the staging threads run (IMPALA_STAGE_PIN): "gpu" (default) the CPUs of the NUMA node
// the device's PCIe link hangs off, so the page-locked blocks they first touch and fill sit
// next to the DMA engines that read them; "caller" the calling thread's node; "0" anywhere.
std::vector<int> stage_cpus(int device) {
  const char* pin = std::getenv("IMPALA_STAGE_PIN");
  if (pin && pin[0] == '0') return {};
  if (pin && std::strcmp(pin, "caller") == 0) return impala_host::local_node_cpus();
  char bus[64] = {};
  int node = -1;
  if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) == hipSuccess) {
    for (char* c = bus; *c; ++c) *c = (char)std::tolower((unsigned char)*c);
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
    if (FILE* f = std::fopen(path.c_str(), "r")) {
      if (std::fscanf(f, "%d", &node) != 1) node = -1;
      std::fclose(f);
    }
  } else {
    (void)hipGetLastError();
  }
  return impala_host::local_node_cpus(node);  // (node -1: the caller's)
}

// impala_stage's copies of one host batch in the ring's layout (also run by the staging
// thread's jobs, which must not wait on themselves)
int stage_now(StageRing& r, const impala_batch* b, int slot) {
  using L = impala_host::StageLayout;
  if (!b || !b->obs || !b->actions || !b->rewards || (!r.ppo && !b->discounts) ||
      !b->behaviour_logits)
    return fail(IMPALA_E_INVALID, "null batch pointer");
  CK(hipSetDevice(r.device));
  auto& s = r.slots[slot];
  for (auto st : r.h2d)  // the steps that read the slot have run
    CK(hipStreamWaitEvent(st, s.done, 0));
  const void* src[L::kFields] = {b->obs, b->actions, b->rewards, b->discounts, b->behaviour_logits};
  // the pull kernel reads page-locked, device-mapped host fields (hipHostGetDevicePointer);
  // anything else takes hipMemcpyAsync
  const void* msrc[L::kFields] = {};
  bool mapped = r.small_pull;
  for (int f = 0; f < L::kFields && mapped; ++f) {
    if (!src[f]) continue;
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, const_cast<void*>(src[f]), 0) != hipSuccess || !dp ||
        (((uintptr_t)dp) & 15) != 0) {
      (void)hipGetLastError();
      mapped = false;
    }
    msrc[f] = dp;
  }
  // the small fields first on stream 0 (one pull launch, or a copy each), then obs in
  // contiguous chunks, one per copy stream
  if (mapped) {
    PullArgs pa{};
    for (int f = 1; f < L::kFields; ++f) {
      if (!msrc[f]) continue;
      pa.src[pa.nf] = (const char*)msrc[f];
      pa.dst[pa.nf] = s.mem + r.lay.off[f];
      pa.bytes[pa.nf] = (long long)r.lay.bytes[f];
      ++pa.nf;
    }
    // 8 workgroups, one per XCD: ~100 KB at PCIe latency (one workgroup took 37-42 us,
    // delaying the obs chunk behind it on the stream; rocprofv3 trace, r04hs3)
    h2d_pull_kernel<<<8, 256, 0, r.h2d[0]>>>(pa);
    CK_LAUNCH("h2d_pull");
  } else {
    for (int f = 1; f < L::kFields; ++f)
      if (src[f])
        CK(hipMemcpyAsync(s.mem + r.lay.off[f], src[f], r.lay.bytes[f], hipMemcpyDefault, r.h2d[0]));
  }
  const size_t ob = r.lay.bytes[L::OBS], chunk = (ob / kCopyStreams + 4095) & ~(size_t)4095;
  char* dobs = s.mem + r.lay.off[L::OBS];
  for (int i = 0; i < kCopyStreams; ++i) {
    const size_t o0 = std::min(ob, (size_t)i * chunk), o1 = std::min(ob, o0 + chunk);
    if (o1 > o0) CK(hipMemcpyAsync(dobs + o0, b->obs + o0, o1 - o0, hipMemcpyDefault, r.h2d[i]));
  }
  for (int i = 1; i < kCopyStreams; ++i) {
    CK(hipEventRecord(r.join, r.h2d[i]));
    CK(hipStreamWaitEvent(r.h2d[0], r.join, 0));
  }
  CK(hipEventRecord(s.ready, r.h2d[0]));
  return 0;
}

// Row staging (impala_stage_rows): the batch is B trajectories scattered in host memory (the
// replay's rows), not one collated host batch.  The host's thread pool copies the rows into the
// slot's page-locked block (impala_host::collate_rows) and stage_now's copies follow.  One
// thread's memcpy moves the 15.7 MB of a C2 batch in ~1 ms, over three times the PCIe copy it
// feeds; the pool's threads (IMPALA_STAGE_THREADS, default 8 with the caller) share it.
int stage_rows_now(StageRing& r, const impala_rows* rows, int n, int slot) {
  using L = impala_host::StageLayout;
  CK(hipSetDevice(r.device));
  auto& s = r.slots[slot];
  if (!s.host_blk) {
    void* p = nullptr;  // default flags, as torch's page-locked tensors, which impala_stage copies from
    CK(hipHostMalloc(&p, r.lay.off[L::kFields], hipHostMallocDefault));
    s.host_blk = (char*)p;
  }
  if (!r.pool) {
    int nt = 7;
    if (const char* e = std::getenv("IMPALA_STAGE_THREADS")) nt = std::max(0, std::atoi(e) - 1);
    r.pool = new (std::nothrow) impala_host::HostPool(nt, stage_cpus(r.device));
    if (!r.pool) return fail(IMPALA_E_STATE, "impala_stage_rows: thread pool");
  }
  // the slot's previous copies (out of its host block too) have finished before it is rewritten
  CK(hipEventSynchronize(s.ready));
  const void* const* src[L::kFields] = {rows->obs, rows->actions, rows->rewards,
                                        r.ppo ? nullptr : rows->discounts, rows->behaviour_logits};
  char* hb = s.host_blk;
  impala_host::collate_rows(r.lay, src, n, hb, r.pool);
  const size_t* o = r.lay.off;
  const impala_batch hbat{(const uint8_t*)(hb + o[L::OBS]), (const int64_t*)(hb + o[L::ACTIONS]),
                          (const float*)(hb + o[L::REWARDS]),
                          r.ppo ? nullptr : (const float*)(hb + o[L::DISCOUNTS]),
                          (const float*)(hb + o[L::LOGITS])};
  return stage_now(r, &hbat, slot);
}

// Prime the copy path at init: the learner's staging loop (ImpalaLearner._stage_host) for
// IMPALA_STAGE_PRIME rounds (default 24, 0 = off) in each of two shapes on a page-locked
// scratch batch, with a 250 us spin kernel on a private stream standing in for each step (with
// fewer than two slots there is no such loop, and nothing to prime).  An H2D hipMemcpyAsync is
// given an SDMA engine by the runtime at issue time (hsa_amd_memory_get_preferred_copy_engine /
// copy_engine_status, then hsa_amd_memory_async_copy_on_engine), and the first copy given an
// engine creates that engine's queue inside the call: a 6-9 ms host stall before the copy is
// submitted (HIP + HSA API traces, profiles/r05d; hsa_queue_create alone takes 6-6.5 ms here).
// Which engines a loop gets depends on what is in flight and waiting when it issues (copies
// queued behind the previous step's events), so rounds of copies with nothing to wait for did
// not reach them (r05c, r05e); in the driver's 20-step host-staged pass one such stall landed
// in the timed steps (0.67 ms per step against a 0.30 ms median, profiles/r05a).
int prime_copy_path(StageRing& r) {
  using L = impala_host::StageLayout;
  int rounds = 24;
  if (const char* e = std::getenv("IMPALA_STAGE_PRIME")) rounds = std::max(0, std::atoi(e));
  if (rounds == 0 || r.n_slots < 2) return 0;
  char* scratch = nullptr;
  CK(hipHostMalloc((void**)&scratch, r.lay.off[L::kFields], hipHostMallocDefault));
  std::memset(scratch, 0, r.lay.off[L::kFields]);
  const size_t* o = r.lay.off;
  const impala_batch hb{(const uint8_t*)(scratch + o[L::OBS]), (const int64_t*)(scratch + o[L::ACTIONS]),
                        (const float*)(scratch + o[L::REWARDS]), (const float*)(scratch + o[L::DISCOUNTS]),
                        (const float*)(scratch + o[L::LOGITS])};
  hipStream_t cs = nullptr;
  hipError_t e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
  int st = e == hipSuccess ? stage_now(r, &hb, 0) : (int)e;
  // one round on slot s: wait for its previous copy, stage it, and let the "step" (250 us) that
  // reads slot `rd` follow on cs -- stage_wait, stage, slot_batch, the step, slot_release
  auto prime_round = [&](int s, int rd) {
    e = hipEventSynchronize(r.slots[s].ready);
    if (e == hipSuccess) st = stage_now(r, &hb, s);
    if (st == 0 && e == hipSuccess) e = hipStreamWaitEvent(cs, r.slots[rd].ready, 0);
    if (st == 0 && e == hipSuccess) {
      stage_prime_spin_kernel<<<1, 64, 0, cs>>>(25000);
      e = hipGetLastError();
    }
    if (st == 0 && e == hipSuccess) e = hipEventRecord(r.slots[rd].done, cs);
  };
  // the two-slot loop: stage slot 1 - s while the step on slot s runs ...
  for (int k = 0; k < rounds && st == 0 && e == hipSuccess; ++k)
    prime_round(1 - (k & 1), k & 1);
  // ... then the same rounds over every slot with the host running ahead, as a loop that reads
  // its metrics only every k steps does (DistributedAgent sync_every > 1): the host waits only
  // for a slot's previous copy (the collate's wait before it rewrites the slot's host block), so
  // every copy is queued behind the event of a step still two slots back.  Without this phase
  // that loop met one 7 ms queue-creation stall in its first dozen steps (profiles/r06y).
  for (int k = 0; k < rounds && st == 0 && e == hipSuccess; ++k)
    prime_round(k % r.n_slots, k % r.n_slots);
  if (cs) {
    const hipError_t es = hipStreamSynchronize(cs);
    if (e == hipSuccess) e = es;
  }
  for (auto s : r.h2d) {
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess) e = es;
  }
  // leave the ring as stage_init's allocation loop does: both events recorded (complete) on
  // h2d[0], none referring to work of the private stream about to be destroyed
  for (int i = 0; i < r.n_slots && e == hipSuccess; ++i) {
    e = hipEventRecord(r.slots[i].ready, r.h2d[0]);
    if (e == hipSuccess) e = hipEventRecord(r.slots[i].done, r.h2d[0]);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(r.h2d[0]);
  if (cs) (void)hipStreamDestroy(cs);
  (void)hipHostFree(scratch);
  if (st) return st;
  if (e != hipSuccess)
    return fail((int)e, std::string("impala_stage_init (copy-path priming): ") + hipGetErrorString(e));
  return 0;
}

// impala_stage_init: (re)allocate `nslots` slots for the handle's batch shape on `device`
int stage_init(StageRing& r, int device, const impala_config& cfg, int nslots) {
  using L = impala_host::StageLayout;
  CK(hipSetDevice(device));
  free_slots(r);
  if (!r.h2d[0]) {
    r.device = device;
    r.ppo = cfg.algo == IMPALA_ALGO_PPO;
    r.lay = L((size_t)cfg.batch_size, (size_t)cfg.rollout_length, (size_t)cfg.num_actions);
    // Data-parallel handles (world_size > 1) take the SDMA copies for the small fields: whether
    // every device of a node maps a rank's page-locked buffers is not something this library
    // checks.  IMPALA_H2D_SMALL_PULL=0|1 overrides; =0 is how the single-GPU tests reach the
    // path that data-parallel handles run.
    r.small_pull = cfg.world_size == 1;
    if (const char* e = std::getenv("IMPALA_H2D_SMALL_PULL")) r.small_pull = e[0] == '1';
    if (int st = acquire_h2d(r)) return st;
    CK(hipEventCreateWithFlags(&r.join, hipEventDisableTiming));
  }
  const size_t* o = r.lay.off;
  for (int i = 0; i < nslots; ++i) {
    auto& s = r.slots[i];
    hipError_t e = hipMalloc(&s.mem, o[L::kFields]);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ready, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
    // both events start recorded (complete), so the first stage / slot_batch never waits
    if (e == hipSuccess) e = hipEventRecord(s.ready, r.h2d[0]);
    if (e == hipSuccess) e = hipEventRecord(s.done, r.h2d[0]);
    if (e != hipSuccess) {
      free_slots(r);
      return fail((int)e, std::string("impala_stage_init: ") + hipGetErrorString(e));
    }
    s.dev = impala_batch{(const uint8_t*)(s.mem + o[L::OBS]), (const int64_t*)(s.mem + o[L::ACTIONS]),
                         (const float*)(s.mem + o[L::REWARDS]), (const float*)(s.mem + o[L::DISCOUNTS]),
                         (const float*)(s.mem + o[L::LOGITS])};
  }
  r.n_slots = nslots;
  if (int st = prime_copy_path(r)) {
    free_slots(r);
    return st;
  }
  return 0;
}

}  // namespace
