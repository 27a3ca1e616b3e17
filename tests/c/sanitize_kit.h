/* What every *_sanitize_main.c of this directory opens with: the C headers, CHECK, the message buffer a walk poisons before each call (so that a
 * missing terminator shows) and AT(), an address that is never dereferenced. */
#ifndef SANITIZE_KIT_H
#define SANITIZE_KIT_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); exit(1); } } while (0)

static char err[200] __attribute__((unused));

/* addresses only: integers, so that no pointer arithmetic leaves an object */
#define AT(a) ((const void *)(uintptr_t)(a))

#endif
