"""The facade's one socket-address builder on the CPU (detail::sock_addr, util.cpp).

Every sockaddr_in / sockaddr_in6 the Segmenter, the Reassembler and getInterfaceAndMTU hand
to the kernel comes from it.  A small program linked against libe2sar_amd.so prints the bytes
and the length it returns -- no GPU call is made -- and they are compared with the same
structures built here from socket.inet_pton and struct.
"""
import itertools
import os
import socket
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "e2sar_amd", "lib")

PROG = r"""
#include <cstdio>
#include <cstdlib>
#include "host_common.hpp"
// argv: triples of host, port, v6 -> "ok|bad <len> <hex of the first len bytes>"
int main(int argc, char **argv)
{
    for (int i = 1; i + 2 < argc; i += 3) {
        const auto a = e2sar::detail::sock_addr(argv[i], (uint16_t)atoi(argv[i + 1]), atoi(argv[i + 2]) != 0);
        printf("%s %u ", a.ok ? "ok" : "bad", (unsigned)a.len);
        for (unsigned k = 0; k < a.len; k++) printf("%02x", reinterpret_cast<const unsigned char *>(&a.ss)[k]);
        printf("\n");
    }
    return 0;
}
"""

V4_HOSTS = ["127.0.0.1", "0.0.0.0", "192.168.100.1", ""]
V6_HOSTS = ["::1", "::", "fe80::1", ""]
PORTS = [0, 1, 19522, 65535]
GOOD = [(h, p, False) for h, p in itertools.product(V4_HOSTS, PORTS)] + \
       [(h, p, True) for h, p in itertools.product(V6_HOSTS, PORTS)]
BAD = [("300.1.1.1", 19522, False), ("not-an-ip", 19522, False), ("not-an-ip", 19522, True),
       ("::1", 19522, False), ("127.0.0.1", 19522, True)]


def expected(host, port, v6):
    """struct sockaddr_in (16 bytes) / sockaddr_in6 (28 bytes) as Linux lays them out: the
    family in host order, the port in network order, the address bytes, the rest zero."""
    if v6:
        addr = socket.inet_pton(socket.AF_INET6, host or "::")
        return struct.pack("=H", socket.AF_INET6) + struct.pack("!HI", port, 0) + addr + struct.pack("=I", 0)
    addr = socket.inet_pton(socket.AF_INET, host or "0.0.0.0")
    return struct.pack("=H", socket.AF_INET) + struct.pack("!H", port) + addr + bytes(8)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """Compile the program once, run it once over every case: {(host, port, v6): (ok, len, bytes)}."""
    if not os.path.exists(os.path.join(LIB, "libe2sar_amd.so")):
        pytest.skip("libe2sar_amd.so not built")
    d = tmp_path_factory.mktemp("sockaddr")
    src, exe = d / "sockaddr.cpp", d / "sockaddr"
    src.write_text(PROG)
    r = subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "e2sar_amd", "csrc", "host"), str(src), "-o", str(exe),
                        "-L", LIB, "-le2sar_amd", "-le2sar_hip", f"-Wl,-rpath,{LIB}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = GOOD + BAD
    argv = [str(exe)]
    for host, port, v6 in cases:
        argv += [host, str(port), "1" if v6 else "0"]
    out = subprocess.run(argv, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    got = {}
    for case, line in zip(cases, out):
        okv, ln, *hx = line.split()
        got[case] = (okv == "ok", int(ln), bytes.fromhex(hx[0]) if hx else b"")
    return got


@pytest.mark.parametrize("host,port,v6", GOOD)
def test_sock_addr_matches_inet_pton(built, host, port, v6):
    okv, ln, raw = built[(host, port, v6)]
    want = expected(host, port, v6)
    assert okv
    assert ln == len(want) == (28 if v6 else 16)          # sizeof(sockaddr_in6) / sizeof(sockaddr_in)
    assert raw[:2] == want[:2]                            # family
    assert raw[2:4] == struct.pack("!H", port)            # port, network order
    assert raw == want                                    # address bytes, everything else zero


@pytest.mark.parametrize("host,port,v6", BAD)
def test_sock_addr_rejects_text_of_the_wrong_family(built, host, port, v6):
    assert built[(host, port, v6)][0] is False
