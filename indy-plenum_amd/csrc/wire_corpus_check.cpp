// wire_corpus_check.cpp -- TEST INFRASTRUCTURE: the wire scanner (wire_scan.h, the lane code of
// edv_wire_scan_kernel) over a corpus file on the host CPU, as a stand-alone program meant to
// be built with -fsanitize=address,undefined (Makefile target wire-corpus-check).  Every text is
// copied into a heap block of exactly its length and scanned into another of the same length, so
// a read or write one byte outside either is reported.  Then the corpus as one wire batch -- the
// texts back to back in a heap block of exactly their total length -- through the identifier pass
// (wire_idents.h, the lane code of edv_wire_ident_*_kernel) with a table of 2 n slots and again
// with one just large enough, whose chains wrap.  Every scanned text also goes through the digest
// pass's top-level walk (wire_digest.h, the lane code of edv_wire_digest_kernel) in its exact-size
// block, every prefix of a short one in a block of the prefix's size (a text that ends early must
// not be walked past its end), and every item of the batch block again, where it must give the
// same answer.
//
// --node: the corpus is rxMsgs entries of a node stack.  Every entry, in a heap block of exactly
// its length, goes through the BATCH parse (node_split.h); every message that yields -- a member
// body, or the entry whole -- is copied into a block of exactly its length and unwrapped
// (wire_unwrap.h, the lane code of edv_wire_unwrap_kernel) into another, and the result is
// scanned.  Every entry is also unwrapped whole both as plain text and as an escaped body, and goes
// through the device split's lane code as an emulated wave (node_split_lanes.h,
// node_split_wave_host.h: what edv_node_split_count_kernel and edv_node_split_emit_kernel run), at
// the place in the buffer the entries before it give it; the verdict, the member count, the body
// bytes and every member's span must equal node_split's.  Then every message as cut, as ONE wire
// batch -- the decoded signatures, the serializations back to back and every per-item array in
// heap blocks of exactly their size -- through the work list (wire_once.h, the lane code of
// edv_wire_once_*_kernel): without `once`, and with it at a table of 2 n slots and at one just
// large enough for the live items, whose chains wrap; the lanes must number the live items and
// the distinct (identifier, signature, message) triples, and every item's verdict, gathered and
// scattered with stand-in result words, must be its own.
//
// Corpus file: per text a little-endian uint32 length, then the bytes
// (tools/wire_probe.py --write-corpus FILE / --write-node-corpus FILE write the test corpora).
// Prints the counts; exit status 0 unless the file is malformed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "node_split.h"
#include "node_split_wave_host.h"
#include "wire_digest.h"
#include "wire_idents.h"
#include "wire_once.h"
#include "wire_scan.h"
#include "wire_unwrap.h"

namespace {
struct SerialTable {  // the device's atomics, one item at a time
  uint32_t* owner;
  uint32_t* first;
  uint32_t owner_load(uint32_t s) const { return owner[s]; }
  uint32_t owner_cas(uint32_t s, uint32_t i) const {
    const uint32_t was = owner[s];
    if (was == edv::kIdentEmpty) owner[s] = i;
    return was;
  }
  uint32_t first_load(uint32_t s) const { return first[s]; }
  void first_min(uint32_t s, uint32_t i) const {
    if (i < first[s]) first[s] = i;
  }
};

// The number of distinct identifiers of the status-0 items, or -1 when the table is too small.
long idents(const uint8_t* text, const std::vector<uint64_t>& off, const std::vector<uint8_t>& status,
            const std::vector<uint32_t>& span, uint64_t cap) {
  const uint64_t n = status.size();
  uint32_t* owner = (uint32_t*)malloc(cap * 4);  // (heap blocks of the exact size, as the texts)
  uint32_t* first = (uint32_t*)malloc(cap * 4);
  uint32_t* slot = (uint32_t*)malloc((n ? n : 1) * 4);
  memset(owner, 0xff, cap * 4);
  memset(first, 0xff, cap * 4);
  long nu = 0;
  for (uint64_t k = 0; k < n && nu >= 0; ++k) {
    const uint64_t i = n - 1 - k;  // (any order gives the same answer: the last item first)
    slot[i] = edv::kIdentEmpty;
    if (status[i] != 0 || !edv::wi_span_ok(off.data(), span.data(), i)) continue;
    slot[i] = edv::wi_insert(text, off.data(), span.data(), SerialTable{owner, first}, (uint32_t)cap, (uint32_t)i);
    if (slot[i] == edv::kIdentEmpty) nu = -1;
  }
  for (uint64_t i = 0; i < n && nu >= 0; ++i) nu += edv::wi_flag(slot, first, i);
  free(owner);
  free(first);
  free(slot);
  return nu;
}
// One message through the unwrap and the scan, each buffer a heap block of exactly len bytes.
struct NodeCounts {
  uint64_t cls[3] = {0, 0, 0}, scanned = 0;
};
// What the scan leaves of the messages, for the work list: per message its status, identifier,
// decoded signature and serialization.
struct NodeBatch {
  std::vector<uint8_t> status, sig, msgs;
  std::vector<uint64_t> start, end;
  std::vector<std::string> idr;
};
bool unwrap_message(const uint8_t* body, uint32_t len, uint32_t esc, NodeCounts& c, NodeBatch* batch = nullptr) {
  uint8_t* text = (uint8_t*)malloc(len ? len : 1);
  uint8_t* mid = (uint8_t*)malloc(len ? len : 1);
  uint8_t* out = (uint8_t*)malloc(len ? len : 1);
  memcpy(text, body, len);
  const int cls = edv::wire_unwrap_one((const uint8_t*)text, len, esc, mid);
  bool ok = cls >= 0 && cls <= 2;
  if (ok) {
    ++c.cls[cls];
    if (len <= edv::kWireMaxText) {
      edv::WireItem it;
      memset(&it, 0, sizeof it);
      const int st = edv::wire_scan_one((const uint8_t*)mid, len, out, it);
      if (st == edv::kWireOk) {
        ++c.scanned;
        ok = cls == edv::kUnwrapRequest && it.msg_len <= len && (uint64_t)it.idr_start + it.idr_len <= len;
      }
      if (batch) {
        const bool live = ok && st == edv::kWireOk;
        batch->status.push_back(live ? 0 : 1);
        batch->sig.insert(batch->sig.end(), (const uint8_t*)it.sig, (const uint8_t*)it.sig + 64);
        batch->start.push_back(batch->msgs.size());
        if (live) batch->msgs.insert(batch->msgs.end(), out, out + it.msg_len);
        batch->end.push_back(batch->msgs.size());
        batch->idr.push_back(live ? std::string((const char*)mid + it.idr_start, it.idr_len) : std::string());
      }
    }
  }
  free(text);
  free(mid);
  free(out);
  return ok;
}

// The entry at [ea, ea + len) of the buffer through the emulated wave, against node_split's answer.
bool lanes_equal(const uint8_t* entry, uint64_t ea, uint64_t len, bool split, const std::vector<edv::NodeSpan>& spans) {
  const edv::EntryCount c = edv::lanes_count(entry, ea, ea + len);
  uint64_t bytes = 0;
  for (const edv::NodeSpan& s : spans) bytes += s.len;
  if (c.split != split || c.members != (split ? spans.size() : 1) || c.bytes != (split ? bytes : len)) return false;
  if (!split) return true;
  uint64_t seen = 0, body = 0;
  bool ok = true;
  std::vector<uint8_t> met(spans.size(), 0);
  edv::lanes_emit(entry, ea, ea + len, [&](uint64_t index, uint64_t at_body, uint64_t first) {
    ok = ok && index < spans.size() && !met[index] && first == ea + spans[index].at;
    if (!ok) return;
    met[index] = 1;
    uint64_t before = 0;
    for (uint64_t j = 0; j < index; ++j) before += spans[j].len;
    ok = at_body == before;
    ++seen;
    body += spans[index].len;
  });
  return ok && seen == spans.size() && body == bytes;
}

template <class V>
V* exact(const std::vector<V>& v) {  // a heap block of exactly the vector's bytes
  V* p = (V*)malloc(v.empty() ? 1 : v.size() * sizeof(V));
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(V));
  return p;
}
struct PlainMsg {
  const uint8_t* p;
  uint8_t operator[](uint64_t i) const { return p[i]; }
  uint64_t word64(uint64_t i) const {
    uint64_t v;
    memcpy(&v, p + i, 8);
    return v;
  }
};

// The batch through the work list with a table of cap slots; the number of lanes, or -1 when a
// verdict came back wrong.  Lane j's stand-in verdict is a hash bit of its gathered signature,
// span and key, so an item's scattered bit must equal the same bit of its own.
long once_pass(const NodeBatch& b, const std::vector<uint32_t>& uidx_v, const std::vector<uint32_t>& kid_v, bool once,
               uint64_t cap, uint64_t* give_ups) {
  const uint64_t n = b.status.size(), nu = kid_v.size();
  uint8_t *status = exact(b.status), *msgs = exact(b.msgs);
  uint32_t *sigw = (uint32_t*)exact(b.sig), *uidx = exact(uidx_v), *kid = exact(kid_v);
  std::vector<uint64_t> spans_v(b.start);
  spans_v.insert(spans_v.end(), b.end.begin(), b.end.end());
  uint64_t* spans = exact(spans_v);
  const uint64_t *ms = spans, *me = spans + n;
  uint32_t* owner = (uint32_t*)malloc(cap * 4);
  uint32_t* first = (uint32_t*)malloc(cap * 4);
  uint32_t* slot = (uint32_t*)malloc((n ? n : 1) * 4);
  uint8_t* grp = (uint8_t*)malloc(n ? n : 1);
  memset(owner, 0xff, cap * 4);
  memset(first, 0xff, cap * 4);
  const SerialTable tab{owner, first};
  *give_ups = 0;
  bool ok = true;
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t i = n - 1 - k;  // (the last item first)
    grp[i] = (uint8_t)edv::wo_group(status, uidx, kid, (uint32_t)nu, i);
    ok = ok && (grp[i] == edv::kOnceDead || edv::wo_span_ok(ms, me, b.msgs.size(), i));
    slot[i] = edv::kIdentEmpty;
    if (once && ok && grp[i] != edv::kOnceDead) {
      slot[i] = edv::wo_insert(sigw, ms, me, PlainMsg{msgs}, uidx, tab, (uint32_t)cap, (uint32_t)cap, (uint32_t)i);
      *give_ups += (uint64_t)(slot[i] == edv::kIdentEmpty);
    }
  }
  long lanes = -1;
  if (ok) {
    std::vector<uint32_t> rank[2] = {std::vector<uint32_t>(n + 1, 0), std::vector<uint32_t>(n + 1, 0)};
    for (uint64_t i = 0; i < n; ++i)
      for (uint32_t g = 0; g < 2; ++g) rank[g][i + 1] = rank[g][i] + edv::wo_flag(grp, slot, first, g + 1, i);
    const uint64_t m[2] = {rank[0][n], rank[1][n]};
    uint32_t* sig_o[2];
    uint64_t *sp_o[2], *words[2];
    uint32_t *rk[2] = {exact(rank[0]), exact(rank[1])};
    for (uint32_t g = 0; g < 2; ++g) {
      sig_o[g] = (uint32_t*)malloc(m[g] ? 64 * m[g] : 1);
      sp_o[g] = (uint64_t*)malloc(m[g] ? 16 * m[g] : 1);
      words[g] = (uint64_t*)calloc((m[g] + 63) / 64 ? (m[g] + 63) / 64 : 1, 8);
    }
    auto verdict = [&](const uint32_t* sg, uint64_t a, uint64_t e, uint32_t u) {
      uint64_t h = 1469598103934665603ull ^ u;
      for (int k = 0; k < 16; ++k) h = (h ^ sg[k]) * 1099511628211ull;
      for (uint64_t p = a; p < e; ++p) h = (h ^ msgs[p]) * 1099511628211ull;
      return (h >> 17) & 1;
    };
    for (uint64_t i = 0; i < n; ++i)
      for (uint32_t g = 0; g < 2; ++g)
        if (edv::wo_flag(grp, slot, first, g + 1, i)) {
          const uint64_t j = rk[g][i];
          edv::wo_emit(sigw, ms, me, i, j, m[g], sig_o[g], sp_o[g]);
          if (verdict(sig_o[g] + 16 * j, sp_o[g][j], sp_o[g][m[g] + j], uidx[i])) words[g][j >> 6] |= 1ull << (j & 63);
        }
    for (uint64_t i = 0; i < n; ++i) {
      const uint32_t bit = edv::wo_bit(grp, slot, first, rk[0], rk[1], words[0], words[1], i);
      const uint32_t want = grp[i] == edv::kOnceDead ? 0 : (uint32_t)verdict(sigw + 16 * i, ms[i], me[i], uidx[i]);
      ok = ok && bit == want;
    }
    lanes = ok ? (long)(m[0] + m[1]) : -1;
    for (uint32_t g = 0; g < 2; ++g) {
      free(sig_o[g]);
      free(sp_o[g]);
      free(words[g]);
      free(rk[g]);
    }
  }
  for (void* p : {(void*)status, (void*)msgs, (void*)sigw, (void*)uidx, (void*)kid, (void*)spans, (void*)owner,
                  (void*)first, (void*)slot, (void*)grp})
    free(p);
  return lanes;
}

// The messages as one batch through the work list; false when it disagrees with the maps here.
bool once_check(const NodeBatch& b) {
  const uint64_t n = b.status.size();
  std::map<std::string, uint32_t> index;
  std::vector<uint32_t> uidx(n, 0), kid;
  for (uint64_t i = 0; i < n; ++i)
    if (b.status[i] == 0 && !index.count(b.idr[i])) {
      const uint32_t j = (uint32_t)index.size();
      index[b.idr[i]] = j;
      kid.push_back(j % 7 == 6 ? edv::kOnceSkip : j % 3 == 0 ? edv::kOnceNoId : j);  // every kind of identifier
    }
  uint64_t live = 0;
  std::map<std::string, int> triples;
  for (uint64_t i = 0; i < n; ++i) {
    uidx[i] = b.status[i] == 0 ? index[b.idr[i]] : (uint32_t)index.size();
    if (b.status[i] != 0 || kid[uidx[i]] == edv::kOnceSkip) continue;
    ++live;
    std::string key((const char*)&uidx[i], 4);
    key.append((const char*)&b.sig[64 * i], 64);
    key.append((const char*)b.msgs.data() + b.start[i], b.end[i] - b.start[i]);
    triples[key] = 1;
  }
  uint64_t cap = 64, tight = 1, gave[3];
  while (cap < 2 * n) cap <<= 1;
  while (tight < live) tight <<= 1;
  const long all = once_pass(b, uidx, kid, false, cap, &gave[0]);
  const long wide = once_pass(b, uidx, kid, true, cap, &gave[1]);
  const long narrow = once_pass(b, uidx, kid, true, tight, &gave[2]);
  printf("work list: items %llu live %llu distinct %llu; lanes %ld, once %ld (table of %llu slots) %ld (of %llu)\n",
         (unsigned long long)n, (unsigned long long)live, (unsigned long long)triples.size(), all, wide,
         (unsigned long long)cap, narrow, (unsigned long long)tight);
  return all == (long)live && wide == (long)triples.size() && narrow == wide && !gave[1] && !gave[2];
}

int node_main(FILE* f) {
  uint64_t entries = 0, split = 0, messages = 0, at = 0, lane_split = 0, lane_members = 0;
  NodeCounts as_cut, whole, escaped;
  NodeBatch batch;
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
    uint8_t* entry = (uint8_t*)malloc(len ? len : 1);
    if (!entry || fread(entry, 1, len, f) != len) {
      fprintf(stderr, "truncated entry\n");
      return 1;
    }
    ++entries;
    std::vector<edv::NodeSpan> spans;
    bool ok = true;
    const bool is_split = edv::node_split(entry, len, spans);
    if (!lanes_equal(entry, at, len, is_split, spans)) {
      fprintf(stderr, "entry %llu: the lane code and node_split disagree\n", (unsigned long long)entries);
      return 1;
    }
    at += len;
    lane_split += is_split;
    lane_members += is_split ? spans.size() : 0;
    if (is_split) {
      ++split;
      for (const edv::NodeSpan& s : spans) {
        ok = ok && s.at + s.len <= len && unwrap_message(entry + s.at, (uint32_t)s.len, 1, as_cut, &batch);
        ++messages;
      }
    } else {
      ok = spans.empty() && unwrap_message(entry, len, 0, as_cut, &batch);
      ++messages;
    }
    ok = ok && unwrap_message(entry, len, 0, whole) && unwrap_message(entry, len, 1, escaped);
    free(entry);
    if (!ok) {
      fprintf(stderr, "entry %llu: a result outside its message\n", (unsigned long long)entries);
      return 1;
    }
  }
  printf("entries %llu split %llu messages %llu\n", (unsigned long long)entries, (unsigned long long)split,
         (unsigned long long)messages);
  printf("lane code: split %llu members %llu, equal to node_split on every entry\n", (unsigned long long)lane_split,
         (unsigned long long)lane_members);
  const NodeCounts* rows[3] = {&as_cut, &whole, &escaped};
  const char* names[3] = {"as cut", "entries whole", "entries as escaped bodies"};
  for (int k = 0; k < 3; ++k)
    printf("%s: request %llu host %llu none %llu scanned %llu\n", names[k], (unsigned long long)rows[k]->cls[0],
           (unsigned long long)rows[k]->cls[1], (unsigned long long)rows[k]->cls[2], (unsigned long long)rows[k]->scanned);
  if (!once_check(batch)) {
    fprintf(stderr, "the work list disagrees with the maps\n");
    return 1;
  }
  return 0;
}
}  // namespace

int main(int argc, char** argv) {
  const bool node = argc == 3 && strcmp(argv[1], "--node") == 0;
  if (argc != 2 && !node) {
    fprintf(stderr, "usage: %s [--node] CORPUS\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[argc - 1], "rb");
  if (!f) {
    perror(argv[argc - 1]);
    return 2;
  }
  if (node) {
    const int r = node_main(f);
    fclose(f);
    return r;
  }
  uint64_t texts = 0, scanned = 0, host = 0, out_bytes = 0, eligible = 0, prefixes = 0;
  std::vector<uint8_t> all, status, elig;
  std::vector<uint64_t> off(1, 0);
  std::vector<uint32_t> span;
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
    const uint32_t el = st == edv::kWireOk ? edv::wd_eligible((const uint8_t*)text, 0, len) : 0;
    eligible += el;
    elig.push_back((uint8_t)el);
    for (uint32_t cut = 0; st == edv::kWireOk && len <= 256 && cut < len; ++cut, ++prefixes) {
      uint8_t* part = (uint8_t*)malloc(cut ? cut : 1);
      memcpy(part, text, cut);
      (void)edv::wd_eligible((const uint8_t*)part, 0, cut);
      free(part);
    }
    all.insert(all.end(), text, text + len);
    off.push_back(all.size());
    status.push_back((uint8_t)st);
    span.push_back(st == edv::kWireOk ? it.idr_start : 0);
    span.push_back(st == edv::kWireOk ? it.idr_len : 0);
    free(text);
    free(out);
  }
  fclose(f);
  printf("texts %llu scanned %llu host %llu serialized bytes %llu\n", (unsigned long long)texts,
         (unsigned long long)scanned, (unsigned long long)host, (unsigned long long)out_bytes);
  uint8_t* batch = (uint8_t*)malloc(all.size() ? all.size() : 1);
  memcpy(batch, all.data(), all.size());
  uint64_t cap = 64;
  while (cap < 2 * texts) cap <<= 1;
  const long nu = idents(batch, off, status, span, cap);
  uint64_t tight = 1;
  while ((long)tight < nu) tight <<= 1;
  const long nu_tight = idents(batch, off, status, span, tight);
  uint64_t differ = 0;
  for (uint64_t i = 0; i < texts; ++i)
    if (status[i] == 0)
      differ += edv::wd_eligible((const uint8_t*)batch, off[i], (uint32_t)(off[i + 1] - off[i])) != elig[i];
  free(batch);
  printf("digest walk: eligible %llu of %llu scanned, %llu prefixes walked\n", (unsigned long long)eligible,
         (unsigned long long)scanned, (unsigned long long)prefixes);
  if (differ) {
    fprintf(stderr, "the digest walk gives %llu items another answer inside the batch\n", (unsigned long long)differ);
    return 1;
  }
  printf("identifiers %ld (table of %llu slots) %ld (of %llu)\n", nu, (unsigned long long)cap, nu_tight,
         (unsigned long long)tight);
  if (nu < 0 || nu_tight != nu) {
    fprintf(stderr, "the identifier pass disagrees with itself\n");
    return 1;
  }
  return 0;
}
