// Hand-over of the per-chunk side states of the stream engine (streams.hip; DESIGN.md section 5, "Side states").
//
// An option of the engine (acoustic activity, phrase spotting, draft transcript, input level) runs a small launch per
// admission and reports a small state "as of the chunk that was just reported".  The launch belongs to a carrier that
// completes later - an encoder group, or a staging slot - named by a KEY that grows with every carrier.  A chunk therefore
// starts with a Pending<V>: the value if it is known already, else the key of the carrier that brings it; when the carrier
// completes, the value is delivered to every place that waits for that key.  A reset bumps the stream's EPOCH, and a value
// planned under an older epoch is dropped on arrival.
//
// Plain C++17 and nothing of the engine or of HIP: tests/host/handover_check.cpp drives this file alone with a host compiler.
#pragma once
#include <vector>

namespace handover {

// the value that belongs to a chunk: ready, or pending on the carrier `key`
template <typename V>
struct Pending {
  bool ready = true;
  long key = 0;
  V v{};
};

// what a carrier records for a span it is going to scan: was the option on, under which epoch was the span planned,
// and does it start the stream's utterance
struct Plan {
  bool on = false;
  long epoch = 0;
  bool restart = false;
};

// one option's state over S streams.  Empty until init(): restart() of an option that was never switched on is a no-op.
template <typename V>
struct Track {
  std::vector<Pending<V>> known;   // per stream: the value of the newest carrier that has delivered
  std::vector<Pending<V>> rep;     // per stream: the value of the last reported chunk (what the readers return)
  std::vector<long> pending;       // per stream: key of the newest carrier with a span of it that has not delivered (0: none)
  std::vector<long> epoch;         // per stream: restarts so far
  std::vector<char> fresh;         // per stream: the next span starts the utterance

  bool allocated() const { return !epoch.empty(); }

  void init(int S) {
    known.assign(S, Pending<V>());
    rep.assign(S, Pending<V>());
    pending.assign(S, 0);
    epoch.assign(S, 0);
    fresh.assign(S, 1);
  }

  // the stream starts over: what is still in flight for it belongs to the old epoch and is dropped when it arrives
  void restart(int s) {
    if (!allocated()) return;
    epoch[s]++;
    known[s] = rep[s] = Pending<V>();
    pending[s] = 0;
    fresh[s] = 1;
  }
  void restart_all() {
    for (size_t s = 0; s < epoch.size(); ++s) restart((int)s);
  }

  // does the next span start the utterance?  Afterwards the one behind it does only if `again` (a final chunk ended it).
  bool take_fresh(int s, bool again = false) {
    const bool f = fresh[s] != 0;
    fresh[s] = again ? 1 : 0;
    return f;
  }
  // a span of the stream is planned now
  Plan plan(int s, bool again = false) { return Plan{true, epoch[s], take_fresh(s, again)}; }

  // the carrier `key` has a span of the stream
  void carry(int s, long key) { pending[s] = key; }

  // Admission: what a new chunk of the stream starts with.  key: the carrier with a span of THIS chunk (0: it has none,
  // or carry() has named it already); done: every carrier up to this key has delivered (0 where carriers complete in any
  // order: only delivery itself clears `pending` then).  A chunk without a span of its own takes its predecessor's value,
  // which may still be in flight.
  Pending<V> admit(int s, long key, long done) {
    if (key) carry(s, key);
    if (pending[s] > done) return Pending<V>{false, pending[s], V{}};
    return known[s];
  }

  // Delivery: the carrier `key` has completed with the value v of a span planned under epoch `ep`.  The value goes to
  // every place that waits for this key: the stream's open job, the jobs queued behind it (member `slot` of each) and rep.
  // The newest key counts for `known` (carriers that complete in order always bring the newest).  False: dropped, the
  // stream has been restarted since the span was planned.
  template <typename Job, typename Queue>
  bool deliver(int s, long key, long ep, const V &v, Job &open, Queue &behind, Pending<V> Job::*slot) {
    if (ep != epoch[s]) return false;
    const Pending<V> k{true, key, v};
    if (key > known[s].key) known[s] = k;
    auto fill = [&](Pending<V> &a) {
      if (!a.ready && a.key == key) a = k;
    };
    fill(open.*slot);
    for (Job &j : behind) fill(j.*slot);
    fill(rep[s]);
    if (pending[s] == key) pending[s] = 0;
    return true;
  }

  // the chunk that carried `v` has been reported
  void report(int s, const Pending<V> &v) { rep[s] = v; }
};

}  // namespace handover
