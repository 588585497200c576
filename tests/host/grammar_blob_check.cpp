// Drives speechcatcher_amd/csrc/grammar_blob.h alone (tests/test_grammar_blob_host.py): every file named on the command
// line is read into a heap block of exactly its size - so that a read past the end is one the address sanitizer sees -
// and handed to grammar_blob::validate.  One line per file: "ok V blank n_states n_arcs start_state" or "bad: <reason>".
#include <cstdio>
#include <cstdlib>

#include "../../speechcatcher_amd/csrc/grammar_blob.h"

int main(int argc, char **argv) {
  for (int a = 1; a < argc; ++a) {
    FILE *f = fopen(argv[a], "rb");
    if (!f) {
      printf("unreadable\n");
      return 2;
    }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    unsigned char *buf = (unsigned char *)malloc(n > 0 ? (size_t)n : 1);
    if (!buf || (n > 0 && fread(buf, 1, (size_t)n, f) != (size_t)n)) {
      printf("unreadable\n");
      return 2;
    }
    fclose(f);
    grammar_blob::Layout L;
    const char *wrong = grammar_blob::validate(buf, n > 0 ? (size_t)n : 0, &L);
    if (wrong)
      printf("bad: %s\n", wrong);
    else
      printf("ok %d %d %d %d %d\n", L.h.V, L.h.blank, L.h.n_states, L.h.n_arcs, L.h.start_state);
    free(buf);
  }
  return 0;
}
