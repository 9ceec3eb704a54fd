// The element loop of the Snappy decoders of snappy_decode.hip, included into each kernel that runs it: decompress_kernel (both
// instantiations) and the block route's decompress_blocks_kernel.  As text and not as a function on purpose: the loop is a
// chain of a few hundred mostly scalar instructions whose pace moved by 4 - 7 % on the MI355X when the same statements reached
// the one-wave kernel through a __forceinline__ function (the instruction selection around the window refill differs by four
// instructions and the loop lands 8 bytes elsewhere; profiles/visindex_device_decode.md).  Included, the kernel's code is what
// it was.
//
// In scope at the point of inclusion: sp (the stream's first byte), n (the end of the input to read, as a stream position),
// p (int64_t, where to start: 0 in front of a preamble), dp (the first output byte), expected (bytes to write), ring (kRing bytes
// of LDS, this wave's), lane, o (int64_t, 0), rc (int, 0) and a constexpr bool kPreamble -- true: sp opens with the stream's
// preamble; false: the elements of one block start at p (n is then the block's end, dp its first byte, expected its size: an
// offset is checked against the bytes written in this block and a copy only ever reads this wave's own stores).  Leaves rc: 0 or
// snappy_core.h's code.
    const int64_t mis = (int64_t)((uintptr_t)sp & 3);

    // the word at stream position rel (rel + mis is a multiple of 4: an aligned load); bytes outside [0, n) read as zero
    auto fetch = [&](int64_t rel) -> uint32_t {
        if (rel >= 0 && rel + 4 <= n) return *(const uint32_t *)(sp + rel);
        uint32_t v = 0;
        for (int j = 0; j < 4; ++j)
            if (rel + j >= 0 && rel + j < n) v |= (uint32_t)sp[rel + j] << (8 * j);
        return v;
    };
    // A window register is settled the moment it is loaded: the empty asm statement makes the load's result a use, so the wait
    // for it stands HERE, once per 256 input bytes, and no load is ever in flight across the element loop -- where the compiler
    // would otherwise have to drain the memory queue (the wave's output stores with it) in front of every element.
    auto settle = [](uint32_t &v) { asm volatile("" : "+v"(v)); };
    int64_t wbase = p - ((p + mis) & 3);                         // stream position of lane 0's word of W (wave-uniform)
    uint32_t W = fetch(wbase + 4 * lane), Wn = fetch(wbase + 256 + 4 * lane);
    settle(W);
    settle(Wn);
    // word j (wave-uniform, < 128) of the window
    auto word = [&](int j) -> uint32_t {
        const int ju = __builtin_amdgcn_readfirstlane(j);
        return (uint32_t)(ju < 64 ? __builtin_amdgcn_readlane((int)W, ju) : __builtin_amdgcn_readlane((int)Wn, ju - 64));
    };
    // the (at least 5) bytes at window position k (wave-uniform, < 256)
    auto peek = [&](int k) -> uint64_t {
        const int ku = __builtin_amdgcn_readfirstlane(k);
        const uint64_t two = (uint64_t)word(ku >> 2) | (uint64_t)word((ku >> 2) + 1) << 32;
        return two >> (8 * (ku & 3));
    };

    if (kPreamble) {
        rc = parse_preamble(peek((int)(p - wbase)), n, expected);
        if (rc > 0) {
            p = rc;
            rc = 0;
        }
    }
    while (rc == 0 && p < n) {
        if (o == expected) {
            rc = kErrTrailing;
            break;
        }
        while (p - wbase >= 256) {
            if (p - wbase >= 512) {                              // a long literal went by: seat the window anew
                wbase = p - ((p + mis) & 3);
                W = fetch(wbase + 4 * lane);
            } else {
                wbase += 256;
                W = Wn;
            }
            Wn = fetch(wbase + 256 + 4 * lane);
            settle(W);
            settle(Wn);
        }
        const int k = (int)(p - wbase);
        Element e;
        rc = parse_element(peek(k), n - p, e);
        if (rc == 0) rc = check_element(e, n - p, o, expected);
        if (rc != 0) break;
        const int64_t len = e.len;
        if (e.literal) {
            if (len <= 64) {                                     // out of the window: k + head + len <= 255 + 5 + 64
                const int kk = k + e.head + lane, j = kk >> 2;
                const uint32_t a = (uint32_t)__shfl((int)W, j & 63), b = (uint32_t)__shfl((int)Wn, j & 63);
                const uint8_t byte = (uint8_t)((j < 64 ? a : b) >> (8 * (kk & 3)));
                if (lane < len) {
                    dp[o + lane] = byte;
                    ring[(uint32_t)(o + lane) & kRingMask] = byte;
                }
            } else {
                for (int64_t done = 0; done < len; done += 64) {
                    const int64_t i = done + lane;
                    if (i < len) {
                        const uint8_t byte = sp[p + e.head + i];
                        dp[o + i] = byte;
                        ring[(uint32_t)(o + i) & kRingMask] = byte;
                    }
                }
            }
            p += e.head + len;
        } else if (e.offset <= kRing) {                          // a copy of 1 .. 64 bytes out of the ring: one step
            const int rem = e.offset >= len ? lane : lane % (int)e.offset;
            uint8_t byte = 0;
            if (lane < len) byte = ring[(uint32_t)(o - e.offset + rem) & kRingMask];
            wave_lds_fence();
            if (lane < len) {
                dp[o + lane] = byte;
                ring[(uint32_t)(o + lane) & kRingMask] = byte;
            }
            p += e.head;
        } else {                                                 // ... from further back: the wave's own stores, out of global memory
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // every store of this wave has been acknowledged
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            if (lane < len) {
                const uint8_t byte = dp[o - e.offset + lane];    // offset > kRing >= len: source and target apart
                dp[o + lane] = byte;
                ring[(uint32_t)(o + lane) & kRingMask] = byte;
            }
            p += e.head;
        }
        o += len;
        wave_lds_fence();
    }
    if (rc == 0 && o < expected) rc = kErrShort;
