// tests/buf_check.cpp -- stand-alone check of DevBuf (nbldpc_amd/csrc/nbl_buf.h), built with the host sanitizers by `make buf_check`
// in nbldpc_amd/csrc and run by tests/test_buf.py.  Without a device every allocation fails and the failure contract is checked;
// with one the growth contract is.  Prints "ok fail" or "ok grow"; any broken expectation names itself and exits 1.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include "nbl_buf.h"

#define EXPECT(c)                                                                  \
	do {                                                                           \
		if (!(c)) { printf("line %d: %s does not hold\n", __LINE__, #c); exit(1); } \
	} while (0)

// The leak check at exit sees host malloc only: DevBuf owns none, and what the HIP runtime keeps for the life of the process is not
// this program's to free.  Address and undefined-behaviour checks stay on.
extern "C" const char *__asan_default_options() { return "detect_leaks=0"; }

template <typename B> static bool check(const char *what)
{
	std::string err;
	B b;
	EXPECT(b.p == nullptr && b.size == 0);
	EXPECT(b.grow(err, 0) == NBL_OK && b.p == nullptr && err.empty()); // nothing asked, nothing done
	if (b.grow(err, 4096) != NBL_OK) {
		EXPECT(b.p == nullptr && b.size == 0 && !err.empty());
		const std::string first = err;
		err.clear();
		EXPECT(b.grow(err, 4096) == NBL_ERR_HIP && b.p == nullptr && b.size == 0 && err == first);
		b.release();
		b.release();
		EXPECT(b.p == nullptr && b.size == 0);
		printf("%s: allocation fails here: %s\n", what, first.c_str());
		return false; // (and the destructor runs on an empty buffer)
	}
	EXPECT(b.p != nullptr && b.size == 4096 && err.empty());
	auto *const p0 = b.p;
	EXPECT(b.grow(err, 1000) == NBL_OK && b.p == p0 && b.size == 4096); // a smaller request keeps what is there
	EXPECT(b.grow(err, 4096) == NBL_OK && b.p == p0 && b.size == 4096);
	EXPECT(b.grow(err, 4097) == NBL_OK && b.p != nullptr && b.size == 4097); // exact, not geometric
	auto *const p1 = (decltype(b.p))b; // the implicit view is the pointer
	EXPECT(p1 == b.p);
	B c(std::move(b)); // a move hands the allocation over and leaves nothing behind
	EXPECT(b.p == nullptr && b.size == 0 && c.p == p1 && c.size == 4097);
	B e;
	EXPECT(e.grow(err, 64) == NBL_OK);
	e = std::move(c); // (frees e's own 64 bytes first)
	EXPECT(c.p == nullptr && c.size == 0 && e.p == p1 && e.size == 4097);
	e.release();
	EXPECT(e.p == nullptr && e.size == 0);
	e.release();
	EXPECT(e.grow(err, 128) == NBL_OK && e.size == 128); // usable again after a release; freed by the destructor
	return true;
}

int main()
{
	const bool dev = check<DevBuf<double>>("device"), host = check<HostBuf<int>>("pinned host");
	EXPECT(dev == host);
	printf(dev ? "ok grow\n" : "ok fail\n");
	return 0;
}
