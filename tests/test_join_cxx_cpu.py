"""CPU-side compile check of InnerJoin's C++ surface (hipcc -fsyntax-only
builds the test TU without a GPU): t9::InnerJoin must instantiate for host
items (pairs, tuples, two different item types), device PODs with signed
keys and plain u64 items, and be hoisted into t9::."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_join_surface_compiles():
    r = subprocess.run(
        ["hipcc", "-O0", "-std=c++17", "-fsyntax-only",
         "-I" + os.path.join(REPO, "include"),
         os.path.join(REPO, "tests", "cxx", "join_test.cpp")],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_non_integral_key_is_refused_at_compile_time(tmp_path):
    src = tmp_path / "bad_key.cpp"
    src.write_text(
        "#include <t9/dia.hpp>\n"
        "void f(t9::Context& ctx) {\n"
        "    auto d = t9::FromVector(ctx, std::vector<uint64_t>{1, 2});\n"
        "    auto k = [](uint64_t x) { return (double)x; };\n"
        "    t9::InnerJoin(d, d, k, k,\n"
        "                  [](uint64_t a, uint64_t b) { return a + b; });\n"
        "}\n")
    r = subprocess.run(
        ["hipcc", "-O0", "-std=c++17", "-fsyntax-only",
         "-I" + os.path.join(REPO, "include"), str(src)],
        capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "integral keys" in r.stderr
