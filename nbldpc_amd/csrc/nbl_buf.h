// nbldpc_amd/csrc/nbl_buf.h -- the one owner of a device (or pinned host) allocation of the host layer: pointer and size in bytes.
// Host-only.  Growth is exact, never geometric: nbl_workspace_bytes is the sum of sizes and is asserted to the byte.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include "../../include/nbldpc.h"

#pragma GCC visibility push(hidden)
template <typename T, bool Pinned = false> struct DevBuf {
	T *p = nullptr;
	size_t size = 0; // bytes

	DevBuf() = default;
	DevBuf(const DevBuf &) = delete;
	DevBuf &operator=(const DevBuf &) = delete;
	// (moves only so that a group of buffers is dropped by assigning a fresh group: `d->tx = Tx()`)
	DevBuf(DevBuf &&o) noexcept : p(o.p), size(o.size) { o.p = nullptr; o.size = 0; }
	DevBuf &operator=(DevBuf &&o) noexcept
	{
		if (this != &o) { release(); p = o.p; size = o.size; o.p = nullptr; o.size = 0; }
		return *this;
	}
	~DevBuf() { release(); }

	operator T *() const { return p; }

	void release()
	{
		if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
		p = nullptr;
		size = 0;
	}

	// At least `bytes`: kept as it is when it already holds them, else freed and allocated anew with exactly `bytes` (the contents
	// are not carried over).  On failure it holds nothing, `err` names the call (the text of HIP_TRY_E) and NBL_ERR_HIP comes back.
	nbl_status grow(std::string &err, size_t bytes)
	{
		if (bytes <= size) return NBL_OK;
		release();
		const hipError_t e = Pinned ? hipHostMalloc((void **)&p, bytes, hipHostMallocDefault) : hipMalloc((void **)&p, bytes);
		if (e != hipSuccess) {
			p = nullptr;
			err = std::string(Pinned ? "hipHostMalloc" : "hipMalloc") + "(" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e);
			return NBL_ERR_HIP;
		}
		size = bytes;
		return NBL_OK;
	}
};
template <typename T> using HostBuf = DevBuf<T, true>; // pinned host memory
#pragma GCC visibility pop
