// reg_columns_main.cpp -- reg_columns.h in the open: the table first, one line per column, then one answer per line of input.
//   rows n | bytes elem n | cap capacity n_old n_new
// Host code with its own main (tests/test_reg_columns.py builds it under AddressSanitizer and UBSan).
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "reg_columns.h"

using namespace posevo;

int main()
{
    for (const RegColumn& c : REG_COLUMN) printf("column %s %u %u %d\n", c.name, c.elem, (unsigned)c.group, c.fill);
    printf("groups %u\n", REG_ALL_GROUPS);
    char op[16];
    while (scanf("%15s", op) == 1) {
        uint64_t a = 0, b = 0, c = 0;
        if (!strcmp(op, "rows") && scanf("%" SCNu64, &a) == 1) printf("%" PRIu64 "\n", reg_rows(a));
        else if (!strcmp(op, "bytes") && scanf("%" SCNu64 " %" SCNu64, &a, &b) == 2) printf("%" PRIu64 "\n", reg_column_bytes(a, b));
        else if (!strcmp(op, "cap") && scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &c) == 3)
            printf("%" PRIu64 "\n", reg_grown_capacity(a, b, c));
        else return 1;
    }
    return 0;
}
