// fps_dd_unit.cpp — the dependency-descriptor frame-rate calculator on the
// host: fps_dd_device.h (the state and the step k_ing_fps_dd runs) over its
// 256-entry scalar stand-in for the wave, built with the host compiler,
// -ffp-contract=off and the address + undefined-behaviour sanitizers
// (make fps_dd_unit).  The header's invariant (every chain member lies inside
// the window) is an abort here.
//
//   fps_dd_unit <script>      ("-": standard input)
//
// A script file holds any number of scripts:
//   S <clockRate>                                   a new stream, NewFrameRateCalculatorDD's state
//   P <fn> <ts> <spatial> <temporal> <n> <diff>*n   one packet with a descriptor that reaches doFpsCalc
//   M <spatial> <temporal>                          SetMaxLayer
// and the program answers one line per line: "S", or the full state
//   <ret> <calculated> | <baseFn> <hasBase> <completed> <maxSpatial> <maxTemporal> <resets>
//   | <present word:016x>*4 | <first slot or -1>*12 | <second slot or -1>*12
//   | <chain word:016x>*4 for each of the 12 layers | <rate bits:08x>*12
// (ret 0 after M), which tests/test_fps_dd_cpu.py compares with
// tests/fps_dd_lib.PyFpsDD.
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#define LKF_FPSDD_ASSERT(c)                                                        \
  do {                                                                             \
    if (!(c)) {                                                                    \
      fprintf(stderr, "fps_dd_unit: invariant broken: %s (line %d)\n", #c, __LINE__); \
      abort();                                                                     \
    }                                                                              \
  } while (0)
#include "fps_dd_device.h"

using namespace lkf;

static uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

struct ListDiffs {
  const std::vector<uint32_t> &v;
  size_t i = 0;
  uint32_t size() const { return uint32_t(v.size()); }
  uint32_t next() { return v[i++]; }
};

static void init(fpsdd::State &s, uint32_t clock) {
  memset(&s, 0, sizeof(s));
  s.kind = fpsdd::KIND_DD;
  s.clockRate = clock;
  fpsdd::set_max_layer(s.h, 2, 3);  // DefaultMaxLayerSpatial / Temporal (fps.go:340-341)
}

static void show(const fpsdd::State &s, bool ret) {
  const fpsdd::Head &h = s.h;
  fpsdd::HostWin w{const_cast<uint32_t *>(s.ts), const_cast<uint16_t *>(s.chain), const_cast<uint8_t *>(s.layer)};
  printf("%d %u | %u %u %u %u %u %u |", ret ? 1 : 0, s.calculated, unsigned(h.baseFn), unsigned(h.hasBase),
         unsigned(h.completed), unsigned(h.maxSpatial), unsigned(h.maxTemporal), h.resets);
  for (int j = 0; j < fpsdd::kWords; j++) printf(" %016" PRIx64, h.present[j]);
  printf(" |");
  for (int l = 0; l < fpsdd::kLayers; l++)
    printf(" %d", (h.has >> l) & 1 ? int(fpsdd::byte_of(h.first[l / 4], l % 4)) : -1);
  printf(" |");
  for (int l = 0; l < fpsdd::kLayers; l++)
    printf(" %d", (h.has >> l) & 1 ? int(fpsdd::byte_of(h.second[l / 4], l % 4)) : -1);
  printf(" |");
  for (int l = 0; l < fpsdd::kLayers; l++)
    for (int j = 0; j < fpsdd::kWords; j++) printf(" %016" PRIx64, w.chain_word(l, j));
  printf(" |");
  for (int l = 0; l < fpsdd::kLayers; l++) printf(" %08x", bits(h.rate[l / 4][l % 4]));
  putchar('\n');
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: fps_dd_unit <script | ->\n");
    return 2;
  }
  FILE *in = strcmp(argv[1], "-") ? fopen(argv[1], "r") : stdin;
  if (!in) {
    perror(argv[1]);
    return 2;
  }
  // (on the heap: the sanitizer sees a window access past the state's end)
  std::unique_ptr<fpsdd::State> st(new fpsdd::State);
  memset(st.get(), 0, sizeof(fpsdd::State));
  std::vector<char> line(1 << 16);
  long lineNo = 0;
  while (fgets(line.data(), int(line.size()), in)) {
    lineNo++;
    if (line[0] == 'S') {
      unsigned clock = 0;
      if (sscanf(line.data() + 1, "%u", &clock) != 1) {
        fprintf(stderr, "line %ld: bad stream\n", lineNo);
        return 2;
      }
      init(*st, clock);
      puts("S");
    } else if (line[0] == 'M') {
      unsigned s = 0, t = 0;
      if (!st->kind || sscanf(line.data() + 1, "%u %u", &s, &t) != 2 || s > 255 || t > 255) {
        fprintf(stderr, "line %ld: bad max layer\n", lineNo);
        return 2;
      }
      fpsdd::set_max_layer(st->h, s, t);
      show(*st, false);
    } else if (line[0] == 'P') {
      unsigned fn = 0, ts = 0, n = 0;
      int spatial = 0, temporal = 0, used = 0;
      if (!st->kind || sscanf(line.data() + 1, "%u %u %d %d %u%n", &fn, &ts, &spatial, &temporal, &n, &used) != 5 ||
          fn > 0xffff) {
        fprintf(stderr, "line %ld: bad packet\n", lineNo);
        return 2;
      }
      std::vector<uint32_t> diffs;
      const char *p = line.data() + 1 + used;
      for (unsigned k = 0; k < n; k++) {
        unsigned d = 0;
        int m = 0;
        if (sscanf(p, "%u%n", &d, &m) != 1 || d < 1 || d > 4096) {  // (12 bits + 1 on the wire)
          fprintf(stderr, "line %ld: bad frame diff\n", lineNo);
          return 2;
        }
        diffs.push_back(d);
        p += m;
      }
      bool ret = false;
      // doFpsCalc (buffer.go:519): nothing once the stream is calculated; all
      // three frameRateCalculator[] entries are this one object
      if (!st->calculated) {
        fpsdd::HostWin w{st->ts, st->chain, st->layer};
        ListDiffs d{diffs};
        // (the kernel's shortcut: where recv_ignores says so, RecvPacket changes nothing)
        const bool ignores = fpsdd::recv_ignores(st->h, uint16_t(fn), spatial, temporal);
        const fpsdd::State before = *st;
        ret = fpsdd::recv(st->h, w, uint16_t(fn), ts, spatial, temporal, d, st->clockRate);
        LKF_FPSDD_ASSERT(!ignores || (!ret && !memcmp(&before, st.get(), sizeof(before))));
        if (ret && st->h.completed) st->calculated = 1;
      }
      show(*st, ret);
    } else if (line[0] != '\n' && line[0] != '#') {
      fprintf(stderr, "line %ld: unknown\n", lineNo);
      return 2;
    }
  }
  if (in != stdin) fclose(in);
  return 0;
}
