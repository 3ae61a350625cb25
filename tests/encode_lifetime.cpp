// encode_lifetime.cpp -- a flattening that fails must not read its problem after the caller let go of it (tests/test_cabi.py
// test_failed_flattening_does_not_outlive_its_problem compiles this file together with host/encode.cpp under the address and undefined-behaviour
// sanitizers and runs it; it needs neither library nor a GPU).
//
//   encode_lifetime FILE.ksp N
//
// FILE.ksp is a KSP1 problem the flattening refuses (ksh::Unsupported) only after it has partitioned the pods into specs -- with 8192 pods or more
// the confirmation of that partition is then still running on a thread of its own.
//   one-shot: N times parse the text and call ksh::encode(std::move(problem), 0): the only owner of the problem unwinds with the exception.
//   cached:   N times ksh::encode(problem, 0, &cache) with the problem held here.
// Every call must throw ksh::Unsupported.  Exit status 0 and "ok" when they all did.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <future>
#include <sstream>

#include "../karpenter_core_amd/host/encode.hpp"

template <class F> static bool refused(const char* road, int i, F&& flatten) {
  try { flatten(); fprintf(stderr, "%s %d: flattened, ksh::Unsupported expected\n", road, i); }
  catch (const ksh::Unsupported&) { return true; }
  catch (const std::exception& e) { fprintf(stderr, "%s %d: %s, ksh::Unsupported expected\n", road, i, e.what()); }
  return false;
}

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s FILE.ksp N\n", argv[0]); return 2; }
  std::ifstream in(argv[1]); std::stringstream ss; ss << in.rdbuf(); const std::string text = ss.str(); const int n = atoi(argv[2]);
  if (text.empty() || n <= 0) { fprintf(stderr, "nothing to do\n"); return 2; }
  bool ok = true;
  for (int i = 0; i < n && ok; ++i) ok = refused("one-shot", i, [&] { ksp::Problem pr = ksp::parse(text); ksh::encode(std::move(pr), 0); });
  { auto pr = std::make_shared<const ksp::Problem>(ksp::parse(text)); ksh::EnvCache cache;
    for (int i = 0; i < n && ok; ++i) ok = refused("cached", i, [&] { ksh::encode(pr, 0, &cache); }); }
  // What the failed flattenings left is torn down on the library's teardown thread, in the order it was handed over: wait until that thread has
  // dropped this marker too, so that the process does not exit under a thread that is still at work.
  std::promise<void> drained;
  ksh::dispose_later(std::shared_ptr<const void>(&drained, [](const void* p) { ((std::promise<void>*)p)->set_value(); }));
  drained.get_future().wait();
  if (ok) printf("ok\n");
  return ok ? 0 : 1;
}
