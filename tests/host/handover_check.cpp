// Stand-alone check of speechcatcher_amd/csrc/handover.h (tests/test_handover_host.py compiles and runs it): the templates
// driven by a scripted, seeded schedule of the events the stream engine has - admit a chunk with or without a span of its
// own, complete a carrier, report the oldest chunk, reset an idle stream - against a straight-line model, checked after
// every event.  Pass 1: carriers complete in order (encoder groups; admission knows the newest completed key).  Pass 2:
// at most 4 carriers in flight, completed in any order (the staging slots of the input level; admission passes 0).
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <set>
#include <vector>

#include "handover.h"

using handover::Pending;
using handover::Plan;
using handover::Track;

namespace {

struct Val { int x = -1; };   // -1: the value before anything of the utterance has been scanned

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) {                                                                  \
      std::fprintf(stderr, "%s:%d: event %d: %s\n", __FILE__, __LINE__, g_event, #cond); \
      std::exit(1);                                                                 \
    }                                                                               \
  } while (0)
int g_event = 0;

// what the model expects of a place that holds a Pending: the value of the latest span planned for the stream, in the same
// epoch, when the place took its value - ready exactly when the carrier `key` of that span has completed (0: no span yet)
struct Want { long key = 0; int x = -1; };
struct Job { Pending<Val> a; Want w; };
struct Span { int s; long epoch; int x; };
struct Carrier { long key; std::vector<Span> spans; };

constexpr int S = 3, DEPTH = 3, EVENTS = 300;

struct Sim {
  bool in_order;
  unsigned rng;
  Track<Val> tr;
  // the engine's side: per stream the open job and the queue behind it, the carriers in flight
  std::vector<Job> open{S};
  std::vector<bool> is_open = std::vector<bool>(S, false);
  std::vector<std::deque<Job>> behind{S};
  std::deque<Carrier> flying;
  long key_next = 1, done_upto = 0;
  int value_next = 100;
  // the model: per stream the latest span of the epoch, the epoch, whether the next span starts the utterance, and what
  // the last reported chunk carried; the keys that have completed
  std::vector<Want> latest{S}, rep{S};
  std::vector<long> epoch = std::vector<long>(S, 0);
  std::vector<bool> fresh = std::vector<bool>(S, true);
  std::set<long> completed;
  int n_pending_reports = 0, n_stale = 0, n_waits_for_predecessor = 0, n_resets = 0, n_reports = 0;

  Sim(bool ordered, unsigned seed) : in_order(ordered), rng(seed) { tr.init(S); completed.insert(0); }
  unsigned rnd(unsigned n) { return ((rng = rng * 1664525u + 1013904223u) >> 8) % n; }
  int outstanding(int s) const { return (is_open[s] ? 1 : 0) + (int)behind[s].size(); }

  void check_place(const Pending<Val> &a, const Want &w) {
    CHECK(a.ready == (completed.count(w.key) != 0));   // ready when the carrier has completed, and not before
    if (a.ready) CHECK(a.v.x == w.x);
    else CHECK(a.key == w.key);
  }
  void check_all() {
    for (int s = 0; s < S; ++s) {
      if (is_open[s]) check_place(open[s].a, open[s].w);
      for (const Job &j : behind[s]) check_place(j.a, j.w);
      check_place(tr.rep[s], rep[s]);
      CHECK(tr.epoch[s] == epoch[s] && (tr.fresh[s] != 0) == fresh[s]);
    }
  }

  // one admission: a chunk for every stream of a random subset that has room; each with a span of its own or without
  void admit() {
    std::vector<int> with, without;
    for (int s = 0; s < S; ++s)
      if (outstanding(s) < DEPTH && rnd(2)) (rnd(5) < 3 ? with : without).push_back(s);
    if (!in_order && flying.size() >= 4) {   // every slot is taken: no new carrier
      without.insert(without.end(), with.begin(), with.end());
      with.clear();
    }
    long key = 0;
    if (!with.empty()) {
      key = key_next++;
      Carrier c{key, {}};
      for (int s : with) {
        const Plan p = tr.plan(s);
        CHECK(p.on && p.epoch == epoch[s] && p.restart == fresh[s]);
        fresh[s] = false;
        latest[s] = Want{key, value_next++};
        c.spans.push_back(Span{s, p.epoch, latest[s].x});
        if (!in_order) tr.carry(s, key);   // (the level names its ticket when the job is planned)
      }
      flying.push_back(c);
    }
    auto start = [&](int s, bool own) {
      Job j;
      j.a = tr.admit(s, own && in_order ? key : 0, in_order ? done_upto : 0);
      j.w = latest[s];
      if (!own && !completed.count(j.w.key)) n_waits_for_predecessor++;
      if (is_open[s]) behind[s].push_back(j);
      else { open[s] = j; is_open[s] = true; }
    };
    for (int s : with) start(s, true);
    for (int s : without) start(s, false);
  }

  void complete() {
    if (flying.empty()) return;
    const size_t at = in_order ? 0 : rnd((unsigned)flying.size());
    const Carrier c = flying[at];
    flying.erase(flying.begin() + (long)at);
    for (const Span &sp : c.spans) {
      const Pending<Val> known = tr.known[sp.s], r = tr.rep[sp.s];
      const long pend = tr.pending[sp.s];
      const bool took = tr.deliver(sp.s, c.key, sp.epoch, Val{sp.x}, open[sp.s], behind[sp.s], &Job::a);
      CHECK(took == (sp.epoch == epoch[sp.s]));
      if (!took) {   // planned under an older epoch: nothing changes
        n_stale++;
        CHECK(tr.known[sp.s].ready == known.ready && tr.known[sp.s].key == known.key && tr.known[sp.s].v.x == known.v.x);
        CHECK(tr.rep[sp.s].ready == r.ready && tr.rep[sp.s].key == r.key && tr.rep[sp.s].v.x == r.v.x);
        CHECK(tr.pending[sp.s] == pend);
      }
    }
    completed.insert(c.key);
    if (in_order) done_upto = c.key;
  }

  void report(int s) {
    if (!is_open[s]) return;
    tr.report(s, open[s].a);
    rep[s] = open[s].w;
    n_reports++;
    if (!open[s].a.ready) n_pending_reports++;
    if (behind[s].empty()) is_open[s] = false;
    else { open[s] = behind[s].front(); behind[s].pop_front(); }
  }

  // (a stream is reset with nothing outstanding: its chunks are reported first, pending or not)
  void reset(int s) {
    while (is_open[s]) report(s);
    tr.restart(s);
    epoch[s]++;
    fresh[s] = true;
    latest[s] = rep[s] = Want();
    n_resets++;
    CHECK(tr.rep[s].ready && tr.rep[s].v.x == -1 && tr.known[s].v.x == -1 && tr.pending[s] == 0);   // the initial value
  }

  void run() {
    for (g_event = 0; g_event < EVENTS; ++g_event) {
      const unsigned e = rnd(10);
      if (e < 4) admit();
      else if (e < 6) complete();
      else if (e < 9) report((int)rnd(S));
      else reset((int)rnd(S));
      check_all();
    }
    while (!flying.empty()) { complete(); check_all(); }
    for (int s = 0; s < S; ++s) CHECK(tr.rep[s].ready);
    // the schedule met the cases it is about
    CHECK(n_reports >= 50 && n_pending_reports >= 5 && n_stale >= 5 && n_waits_for_predecessor >= 5 && n_resets >= 10);
    std::printf("%s: %d reports (%d still pending), %d stale deliveries, %d chunks behind an unfinished carrier, %d resets\n",
                in_order ? "in order" : "any order", n_reports, n_pending_reports, n_stale, n_waits_for_predecessor, n_resets);
  }
};

}  // namespace

int main() {
  Track<Val> never;   // an option that was never switched on: restart is a no-op
  never.restart(0);
  never.restart_all();
  if (never.allocated()) return 1;
  Sim(true, 20240607u).run();
  Sim(false, 7u).run();
  std::puts("handover ok");
  return 0;
}
