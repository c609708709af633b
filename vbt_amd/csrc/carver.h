// One allocation as regions that each begin on an ALIGN-byte boundary (host code only): name every region once with add<T>(count),
// allocate bytes() - or padded_bytes(), where the last region is rounded up as well - and ptr(blob, region) is where it lies.
#pragma once
#include <cstddef>
#include <cstdint>

namespace vbt {

template <size_t ALIGN>
class Carver {
  static_assert(ALIGN > 0 && (ALIGN & (ALIGN - 1)) == 0, "a power of two");
  size_t total = 0;

 public:
  static size_t align(size_t v) { return (v + ALIGN - 1) & ~(ALIGN - 1); }
  template <class T> struct Region { size_t at; };
  template <class T> Region<T> add(size_t count) {
    const Region<T> r{align(total)};
    total = r.at + count * sizeof(T);
    return r;
  }
  size_t bytes() const { return total; }
  size_t padded_bytes() const { return align(total); }
  template <class T> static T* ptr(uint8_t* blob, Region<T> r) { return (T*)(blob + r.at); }
};

}  // namespace vbt
