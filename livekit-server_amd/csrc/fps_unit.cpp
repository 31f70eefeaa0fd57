// fps_unit.cpp — the ingress frame-rate calculators on the host: fps_device.h
// (the state and the step k_ing_fps runs) over its 64-entry scalar stand-in
// for the wave, built with the host compiler, -ffp-contract=off and the
// address + undefined-behaviour sanitizers (make fps_unit).
//
//   fps_unit <script>      ("-": standard input)
//
// A script file holds any number of scripts:
//   S <kind> <clockRate>               a new stream (kind 1 VP8, 2 VP9), all calculators zero
//   P <fn> <ts> <temporal> <spatial>   one packet that reaches doFpsCalc
// and the program answers one line per line: "S", or after a packet
//   <ret> <calculated> then per calculator (1 for VP8, 3 for VP9)
//   <present:016x> <first:08x> <second:08x> <baseFn> <hasBase> <completed> <resets> <rate bits x4:08x>
// which tests/test_fps_cpu.py compares with tests/fps_lib.PyFps.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <memory>

#include "fps_device.h"

using namespace lkf;

static uint32_t bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: fps_unit <script | ->\n");
    return 2;
  }
  FILE *in = strcmp(argv[1], "-") ? fopen(argv[1], "r") : stdin;
  if (!in) {
    perror(argv[1]);
    return 2;
  }
  // (on the heap: the sanitizer sees a window access past the state's end)
  std::unique_ptr<fps::State> st(new fps::State);
  memset(st.get(), 0, sizeof(fps::State));
  char line[256];
  long lineNo = 0;
  while (fgets(line, sizeof(line), in)) {
    lineNo++;
    if (line[0] == 'S') {
      unsigned kind = 0, clock = 0;
      if (sscanf(line + 1, "%u %u", &kind, &clock) != 2 || (kind != fps::KIND_VP8 && kind != fps::KIND_VP9)) {
        fprintf(stderr, "line %ld: bad stream\n", lineNo);
        return 2;
      }
      memset(st.get(), 0, sizeof(fps::State));
      st->kind = kind;
      st->clockRate = clock;
      puts("S");
    } else if (line[0] == 'P') {
      unsigned fn = 0, ts = 0;
      int temporal = 0, spatial = 0;
      if (!st->kind || sscanf(line + 1, "%u %u %d %d", &fn, &ts, &temporal, &spatial) != 4 || fn > 0xffff) {
        fprintf(stderr, "line %ld: bad packet\n", lineNo);
        return 2;
      }
      const int nc = st->kind == fps::KIND_VP9 ? fps::kSpatial : 1;
      bool ret = false;
      // doFpsCalc (buffer.go:519): nothing once the stream is calculated
      if (!st->calculated) {
        // VP8: the one calculator whatever ep.Spatial is (buffer.go:522-526);
        // VP9: ep.Spatial selects, anything else is ignored (fps.go:264-267)
        const int c = st->kind == fps::KIND_VP8 ? 0 : spatial;
        if (c >= 0 && c < nc) {
          fps::HostWin w{st->c[c].ts, st->c[c].temporal};
          ret = fps::recv(st->c[c].h, w, uint16_t(fn), ts, temporal, st->clockRate);
        }
        uint8_t done[fps::kSpatial];
        for (int k = 0; k < fps::kSpatial; k++) done[k] = st->c[k].h.completed;
        if (fps::stream_done(st->kind, ret, done)) st->calculated = 1;
      }
      printf("%d %u", ret ? 1 : 0, st->calculated);
      for (int c = 0; c < nc; c++) {
        const fps::Head &h = st->c[c].h;
        printf(" | %016" PRIx64 " %08x %08x %u %u %u %u %08x %08x %08x %08x", h.present, h.first, h.second,
               unsigned(h.baseFn), unsigned(h.hasBase), unsigned(h.completed), h.resets, bits(h.rate[0]),
               bits(h.rate[1]), bits(h.rate[2]), bits(h.rate[3]));
      }
      putchar('\n');
    } else if (line[0] != '\n' && line[0] != '#') {
      fprintf(stderr, "line %ld: unknown\n", lineNo);
      return 2;
    }
  }
  if (in != stdin) fclose(in);
  return 0;
}
