// parse_replica_inbound_reads (csrc/fpx_wire_parse.hpp: ReplicaInbound with the replica's read path) driven on its own:
// built with -fsanitize=address,undefined and run on the CPU by tests/test_replica_inbox_cpu.py.  Every message, every
// proper prefix of it and every single-byte corruption of it is parsed from an exactly-sized heap copy, so that a read
// past the end of a message is caught.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../frankenpaxos_amd/csrc/fpx_wire_parse.hpp"

using namespace fpxw;
typedef std::string Bytes;

static int failures = 0;
#define EXPECT(c)                                               \
  do {                                                          \
    if (!(c)) {                                                 \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);      \
      ++failures;                                               \
    }                                                           \
  } while (0)

static Bytes varint(uint64_t v) {
  Bytes o;
  while (v >= 0x80) o.push_back((char)(v | 0x80)), v >>= 7;
  o.push_back((char)v);
  return o;
}
static Bytes i32(int field, int32_t v) { return varint((uint64_t)field << 3) + varint((uint64_t)(int64_t)v); }
static Bytes sub(int field, const Bytes& body) { return varint(((uint64_t)field << 3) | 2) + varint(body.size()) + body; }
static Bytes command(const Bytes& addr, int32_t pseudonym, int32_t id, const Bytes& payload) {
  return sub(1, sub(1, addr) + i32(2, pseudonym) + i32(3, id)) + sub(2, payload);
}

static bool parse(const Bytes& m, ReplicaMsg* o) {
  uint8_t* heap = (uint8_t*)std::malloc(m.size() ? m.size() : 1);  // exactly the message
  std::memcpy(heap, m.data(), m.size());
  const bool ok = parse_replica_inbound_reads(heap, Reader{heap, heap + m.size()}, o);
  std::free(heap);
  return ok;
}

int main() {
  const Bytes c1 = command("10.0.0.1:9000", 3, 17, "get x"), c2 = command("", 0, -5, Bytes(200, 'k'));
  struct Case { Bytes bytes; int kind, slot, count; int64_t off; int len; };
  std::vector<Case> cases;
  for (int32_t slot : {-1, 0, 5, 300, 2147483647}) {
    for (int member : {2, 3}) {
      const Bytes head = i32(1, slot), inner = head + sub(2, c1), m = sub(member, inner);
      cases.push_back({m, 10 + member, slot, 1, (int64_t)(m.size() - c1.size()), (int)c1.size()});
    }
    for (int member : {5, 6}) {
      const Bytes inner = i32(1, slot) + sub(2, c1) + sub(2, c2) + sub(2, c1), m = sub(member, inner);
      cases.push_back({m, 19 + member, slot, 3, (int64_t)(m.size() - inner.size()), (int)inner.size()});
    }
  }
  {
    const Bytes m = sub(4, sub(1, c2));
    cases.push_back({m, 14, -1, 1, (int64_t)(m.size() - c2.size()), (int)c2.size()});
    const Bytes inner = sub(1, c1) + sub(1, c2), b = sub(7, inner);
    cases.push_back({b, 26, -1, 2, (int64_t)(b.size() - inner.size()), (int)inner.size()});
    const Bytes e = sub(7, "");
    cases.push_back({e, 26, -1, 0, (int64_t)e.size(), 0});
    const Bytes value = sub(2, ""), ch = sub(1, i32(1, 9) + sub(2, value));  // Chosen(9, Noop)
    cases.push_back({ch, 4, 9, -1, (int64_t)(ch.size() - value.size()), (int)value.size()});
  }
  long parsed = 0;
  for (const Case& c : cases) {
    ReplicaMsg o;
    EXPECT(parse(c.bytes, &o));
    EXPECT(o.kind == c.kind && o.slot == c.slot && o.count == c.count && o.value_off == c.off && o.value_len == c.len);
    // unknown fields before and after change nothing but the offset
    const Bytes pre = i32(15, 7) + sub(9, "zz");
    ReplicaMsg p;
    EXPECT(parse(pre + c.bytes + i32(14, 1), &p));
    EXPECT(p.kind == c.kind && p.slot == c.slot && p.count == c.count && p.value_off == c.off + (int64_t)pre.size());
    for (size_t cut = 1; cut < c.bytes.size(); ++cut) {  // the outer length says more than is there
      ReplicaMsg q;
      EXPECT(!parse(c.bytes.substr(0, cut), &q));
      ++parsed;
    }
    for (size_t at = 0; at < c.bytes.size(); ++at)  // whatever the verdict: no read outside the message
      for (int bit : {0x01, 0x80, 0xff}) {
        Bytes d = c.bytes;
        d[at] = (char)(d[at] ^ bit);
        ReplicaMsg q;
        (void)parse(d, &q);
        ++parsed;
      }
  }
  ReplicaMsg o;
  EXPECT(parse("", &o) && o.kind == 0 && o.slot == -1);
  EXPECT(!parse(sub(2, i32(1, 3)), &o));                                   // no command
  EXPECT(!parse(sub(2, sub(2, c1)), &o));                                  // no slot
  EXPECT(!parse(sub(4, ""), &o));                                          // no command
  EXPECT(!parse(sub(2, i32(1, 3) + sub(2, sub(2, "A"))), &o));             // a Command without its command_id
  EXPECT(!parse(sub(5, i32(1, 3) + sub(2, sub(1, sub(1, "a") + i32(2, 1)) + sub(2, "A"))), &o));  // CommandId without client_id
  EXPECT(parse(sub(5, i32(1, 3)), &o) && o.kind == 24 && o.count == 0);    // an empty batch is a message
  // the last member of the oneof wins
  EXPECT(parse(cases[0].bytes + cases.back().bytes, &o) && o.kind == 4 && o.slot == 9 && o.count == -1);
  EXPECT(parse(cases.back().bytes + cases[0].bytes, &o) && o.kind == 12 && o.slot == -1 && o.count == 1 && o.is_noop == -1);
  if (failures) return 1;
  std::printf("replica inbox parser ok: %zu messages, %ld damaged copies\n", cases.size(), parsed);
  return 0;
}
