// wire_corpus_check.cpp -- TEST INFRASTRUCTURE: the wire scanner (wire_scan.h, the lane code of
// edv_wire_scan_kernel) over a corpus file on the host CPU, as a stand-alone program meant to
// be built with -fsanitize=address,undefined (Makefile target wire-corpus-check).  Every text is
// copied into a heap block of exactly its length and scanned into another of the same length, so
// a read or write one byte outside either is reported.
//
// Corpus file: per text a little-endian uint32 length, then the bytes
// (tools/wire_probe.py --write-corpus FILE writes the test corpus in this form).
// Prints the counts; exit status 0 unless the file is malformed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wire_scan.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s CORPUS\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  uint64_t texts = 0, scanned = 0, host = 0, out_bytes = 0;
  for (;;) {
    uint8_t hdr[4];
    const size_t got = fread(hdr, 1, 4, f);
    if (got == 0) break;
    if (got != 4) {
      fprintf(stderr, "truncated length\n");
      return 1;
    }
    const uint32_t len = (uint32_t)hdr[0] | (uint32_t)hdr[1] << 8 | (uint32_t)hdr[2] << 16 | (uint32_t)hdr[3] << 24;
    if (len > (64u << 20)) {
      fprintf(stderr, "implausible length %u\n", len);
      return 1;
    }
    uint8_t* text = (uint8_t*)malloc(len ? len : 1);
    uint8_t* out = (uint8_t*)malloc(len ? len : 1);
    if (!text || !out || fread(text, 1, len, f) != len) {
      fprintf(stderr, "truncated text\n");
      return 1;
    }
    edv::WireItem it;
    memset(&it, 0, sizeof it);
    const int st = edv::wire_scan_one((const uint8_t*)text, len, out, it);
    ++texts;
    if (st == edv::kWireOk) {
      ++scanned;
      out_bytes += it.msg_len;
      if (it.msg_len > len || (uint64_t)it.idr_start + it.idr_len > len) {
        fprintf(stderr, "text %llu: result outside the text\n", (unsigned long long)texts);
        return 1;
      }
    } else {
      ++host;
    }
    free(text);
    free(out);
  }
  fclose(f);
  printf("texts %llu scanned %llu host %llu serialized bytes %llu\n", (unsigned long long)texts,
         (unsigned long long)scanned, (unsigned long long)host, (unsigned long long)out_bytes);
  return 0;
}
