"""csrc/dev_buf.h on a machine without a device: the owner's failure side.  hipMalloc and hipHostMalloc fail there (no device), so
a stand-alone host program can check that a failed alloc / upload / grow returns BDF_ERR_HIP with a message, leaves the owner empty
and the live counters at zero, that empty and moved-from owners move, reset and die safely, and that a std::map of a move-only
struct of owners -- what the row launcher keeps its plans in -- compiles and erases.  With a device the same program's allocations
succeed instead; it then checks the counters' arithmetic and that everything is given back."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesiandatafusion.jl_amd", "csrc")

SRC = r'''
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <utility>
#include "dev_buf.h"

static char g_msg[512] = "";
void bdf_set_error(const char *fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_msg, sizeof(g_msg), fmt, ap); va_end(ap); }

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); fails++; } } while (0)

static bool live_is(int64_t blocks, int64_t bytes) { return g_dev_live_blocks.load() == blocks && g_dev_live_bytes.load() == bytes; }

struct Plan { DevBuf<int> a; DevBuf<double> b; int n = 0; };       // move-only through its members

// rc of an alloc / upload / grow of `bytes` on owner b: the failure side without a device, the success side with one
template <typename B>
static void outcome(int rc, const B &b, size_t bytes, bool have_device)
{
    if (have_device) {
        CHECK(rc == BDF_OK && b && b.get() != nullptr && b.bytes() == bytes && live_is(1, (int64_t)bytes));
    } else {
        CHECK(rc == BDF_ERR_HIP);
        CHECK(strlen(g_msg) > 0 && strstr(g_msg, "failed: ") && strstr(g_msg, "dev_buf.h:"));
        CHECK(!b && b.get() == nullptr && b.bytes() == 0);
        CHECK(live_is(0, 0));
    }
    g_msg[0] = 0;
}

int main()
{
    int ndev = 0;
    const bool have_device = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
    CHECK(live_is(0, 0));
    {
        DevBuf<double> d;
        outcome(d.alloc(100), d, 800, have_device);
        d.reset();
        outcome(d.alloc_bytes(24), d, 24, have_device);
        d.reset();
        outcome(d.upload(std::vector<double>{1.0, 2.0, 3.0}), d, 24, have_device);
        d.reset();
        outcome(d.upload(std::vector<double>{}), d, 16, have_device);          // (the 16-byte minimum)
        d.reset();
        outcome(d.grow(4096), d, 4096, have_device);
        d.reset();
        outcome(d.grow(4096, (hipStream_t) nullptr), d, 4096, have_device);
        if (have_device) { double *was = d.get(); CHECK(d.grow(1024) == BDF_OK && d.get() == was && d.bytes() == 4096); }   // fits: kept
        d.reset();
        CHECK(live_is(0, 0));
        DevBuf<void> v;
        outcome(v.alloc(256), v, 256, have_device);                            // (void counts bytes)
        v.reset();
        DevBuf<int> pinned = DevBuf<int>::pinned(kPinnedMappedCoherent);
        outcome(pinned.alloc(16), pinned, 64, have_device);
        DevBuf<volatile uint64_t> status = DevBuf<volatile uint64_t>::pinned(kPinnedMapped);
        pinned.reset();
        outcome(status.alloc(2), status, 16, have_device);
        status.reset();
        DevBuf<double> rec_host = DevBuf<double>::pinned(kPinnedDefault);
        outcome(rec_host.alloc(3), rec_host, 24, have_device);
    }
    CHECK(live_is(0, 0));
    {   // empty and moved-from owners
        DevBuf<double> a, b(std::move(a));
        CHECK(!a && !b);
        a = std::move(b);
        CHECK(!a && !b);
        DevBuf<double> &self = a;
        a = std::move(self);                                               // (to itself)
        a.reset(); a.reset(); b.reset();
        CHECK(a.release() == nullptr && live_is(0, 0));
        if (have_device) {
            CHECK(a.alloc(10) == BDF_OK);
            double *p = a.get();
            DevBuf<double> c(std::move(a));
            CHECK(!a && c.get() == p && c.bytes() == 80 && live_is(1, 80));
            b = std::move(c);
            CHECK(!c && b.get() == p && live_is(1, 80));
            CHECK(c.alloc(5) == BDF_OK && live_is(2, 120));
            b = std::move(c);                                                  // frees what b held
            CHECK(live_is(1, 40));
            double *q = b.release();
            CHECK(q && !b && live_is(0, 0));
            CHECK(hipFree(q) == hipSuccess);
        }
        DevEvent e, f(std::move(e));
        CHECK((hipEvent_t)e == nullptr && (hipEvent_t)f == nullptr);
    }
    {   // a map of move-only plans
        std::map<int, Plan> plans;
        for (int k = 0; k < 4; k++) {
            Plan p;
            p.n = k;
            if (have_device) { CHECK(p.a.alloc(4) == BDF_OK && p.b.alloc(2) == BDF_OK); }
            else { CHECK(p.a.alloc(4) == BDF_ERR_HIP && p.b.upload(std::vector<double>(2, 0.0)) == BDF_ERR_HIP); }
            plans.emplace(k, std::move(p));
        }
        CHECK(plans.size() == 4 && plans.at(3).n == 3);
        CHECK(have_device ? live_is(8, 4 * 32) : live_is(0, 0));
        for (auto it = plans.begin(); it != plans.end();) it = it->first % 2 ? plans.erase(it) : ++it;
        CHECK(plans.size() == 2);
        CHECK(have_device ? live_is(4, 2 * 32) : live_is(0, 0));
    }
    CHECK(live_is(0, 0));
    printf("%s device=%d failures=%d\n", fails ? "BAD" : "OK", have_device ? 1 : 0, fails);
    return fails ? 1 : 0;
}
'''


def build_program(td, extra=()):
    """the program above, compiled the way test_nonneg_host.py compiles its own: hipcc as a host compiler"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    src, exe = os.path.join(td, "t.cpp"), os.path.join(td, "t")
    open(src, "w").write(SRC)
    subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", *extra, "-I", CSRC, "-I", os.path.join(rocm, "include"),
                    src, "-o", exe, "-L", os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    return exe


@pytest.fixture(scope="module")
def report():
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([build_program(td)], capture_output=True, text=True)
        yield r


def test_owner_program_passes_every_check(report):
    """every CHECK of the program holds: failed alloc / upload / grow return BDF_ERR_HIP, set the message, leave the owner empty and
    the counters at zero; moves, resets and destruction of empty and moved-from owners are safe; the map of move-only plans erases"""
    assert report.returncode == 0, report.stdout + report.stderr
    assert "FAILED" not in report.stdout and report.stdout.startswith("OK "), report.stdout
    assert "failures=0" in report.stdout


def test_the_failure_side_is_what_ran_without_a_device(report):
    """on a machine without a device the program must have taken the failure branches (device=0); with one, the success branches"""
    import torch
    have = torch.cuda.is_available()
    assert ("device=%d" % (1 if have else 0)) in report.stdout, report.stdout
