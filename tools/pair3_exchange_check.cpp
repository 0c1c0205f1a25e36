// Host model of the per-block row-sum exchange of the backward pair launch (medmoe_amd/csrc/pair3.hip): the NTT waves of one caption
// group as threads, the LDS mailboxes as PLAIN memory and the flags as release / acquire atomics (the kernel's s_waitcnt lgkmcnt(0)
// in front of the flag store, and the in-order LDS reads behind the flag read).  Every wave runs the kernel's order of events:
//   for sp < NS: write slot (epoch parity, sp); publish 8 epoch + sp + 1; if sp > 0 finish block sp - 1;      then finish block NS - 1
// where finishing block b waits for all flags >= 8 epoch + b + 1 and reads every wave's slot of b.  A slot holds a tag
// (epoch, block, writer); a reader checks the tag it finds.  Built with the thread sanitizer (`make check-exchange`): a slot overwritten
// while a partner may still read it, or read before it was written, is a data race on plain memory and is reported; a deadlock would
// not finish.  usage: pair3_exchange_check [epochs]
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

constexpr int NS = 7, MAXW = 5;
struct Group {
  int ntt;
  std::atomic<int> flag[MAXW];
  long slot[2][MAXW][NS];          // [epoch parity][wave][block], plain memory on purpose
  std::atomic<long> bad{0};
};
static long tag(int epoch, int sp, int w) { return ((long)epoch * NS + sp) * MAXW + w + 1; }

static void finish_block(Group& g, int epoch, int sp) {
  for (int q = 0; q < g.ntt; ++q)
    while (g.flag[q].load(std::memory_order_acquire) < 8 * epoch + sp + 1) std::this_thread::yield();
  for (int q = 0; q < g.ntt; ++q)
    if (g.slot[epoch & 1][q][sp] != tag(epoch, sp, q)) g.bad.fetch_add(1);
}

static void wave(Group& g, int w, int epochs, unsigned seed) {
  for (int epoch = 1; epoch <= epochs; ++epoch)
    for (int sp = 0; sp <= NS; ++sp) {
      seed = seed * 1664525u + 1013904223u;
      if ((seed >> 24) < 48) std::this_thread::yield();          // the waves of a workgroup drift apart
      if (sp < NS) {
        g.slot[epoch & 1][w][sp] = tag(epoch, sp, w);
        g.flag[w].store(8 * epoch + sp + 1, std::memory_order_release);
      }
      if (sp > 0) finish_block(g, epoch, sp - 1);
    }
}

int main(int argc, char** argv) {
  const int epochs = argc > 1 ? atoi(argv[1]) : 300;
  for (int ntt = 2; ntt <= MAXW; ++ntt) {
    Group g;
    g.ntt = ntt;
    for (auto& f : g.flag) f.store(0);
    for (auto& a : g.slot) for (auto& b : a) for (long& c : b) c = 0;
    std::vector<std::thread> th;
    for (int w = 0; w < ntt; ++w) th.emplace_back(wave, std::ref(g), w, epochs, 12345u * (w + 1) + ntt);
    for (auto& t : th) t.join();
    if (g.bad.load()) { printf("NTT %d: %ld wrong tags\n", ntt, g.bad.load()); return 1; }
    printf("NTT %d: %d epochs x %d blocks, every slot read with its own tag\n", ntt, epochs, NS);
  }
  return 0;
}
