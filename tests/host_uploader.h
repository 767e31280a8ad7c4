// TEST INFRASTRUCTURE ONLY -- the `Up` of smj_load_model (csrc/smj_model_load.h) for host programs: every table is copied into malloc'd
// memory that the caller frees through `keep`.  `bytes`, when set, remembers the byte size of every upload by its address.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <map>
#include <vector>
struct HostUploader {
  std::vector<void*>* keep;
  std::map<const void*, size_t>* bytes = nullptr;
  template <class T>
  const T* put(const std::vector<T>& h) {
    T* p = (T*)malloc(h.size() * sizeof(T) + 1);
    memcpy(p, h.data(), h.size() * sizeof(T));
    keep->push_back(p);
    if (bytes) (*bytes)[p] = h.size() * sizeof(T);
    return p;
  }
  const float* f32(const std::vector<float>& h) { return put(h); }
  const int* i32(const std::vector<int>& h) { return put(h); }
};
