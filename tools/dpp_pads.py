"""Dev tool: checks, in a hipcc -S listing, the wait states in front of every inline-asm statement that opens with a DPP
instruction (the factorisation steps of csrc/lipmpc_fused_steps.inc after the first).  A VGPR written by a VALU instruction
needs 2 wait states before a DPP instruction reads it (tools/dpp_hazard_test.hip); the compiler cannot see the DPP read
inside the statement, so nothing it places in front of the statement may write a register the statement's DPP
instructions read within 2 wait states of them.  Prints the statements checked and every violation; exit status 1 on any.
    python tools/dpp_pads.py LISTING.s [...]"""
import re
import sys

REG = re.compile(r'v\[(\d+):(\d+)\]|\bv(\d+)\b')


def regs(text):
    out = set()
    for m in REG.finditer(text):
        if m.group(3) is not None:
            out.add(int(m.group(3)))
        else:
            out.update(range(int(m.group(1)), int(m.group(2)) + 1))
    return out


def check(path):
    lines = [l.split(';')[0].strip() for l in open(path).read().split('\n')]
    raw = open(path).read().split('\n')
    n_checked, bad = 0, []
    for i, l in enumerate(raw):
        if ';;#ASMSTART' not in l:
            continue
        body = []
        for k in range(i + 1, len(raw)):
            if ';;#ASMEND' in raw[k]:
                break
            body.append(lines[k])
        if not body or '_dpp' not in body[0]:
            continue                      # the statement opens with its own wait (s_nop) or no DPP read at all
        # DPP source (src0) registers read by the statement before its own first write of them: src0 is the second operand
        read = set()
        for b in body:
            if '_dpp' in b:
                ops = b.split(None, 1)[1].split(',')
                read |= regs(ops[1])
        # walk back over 2 wait states of compiler code
        need, k = 2, i - 1
        while need > 0 and k >= 0:
            s = lines[k]
            k -= 1
            if not s or s.startswith('.') or s.startswith(';'):
                if raw[k + 1].startswith('.LBB'):
                    bad.append((i + 1, 'label (branch target) within 2 wait states'))
                    break
                continue
            m = re.match(r's_nop\s+(\d+)', s)
            if m:
                need -= int(m.group(1)) + 1
                continue
            if s.startswith('s_') and not s.startswith('s_nop'):
                need -= 1                 # an SALU instruction is one wait state and writes no VGPR
                continue
            if ';;#ASMEND' in raw[k + 1]:
                need -= 1
                continue
            parts = s.split(None, 1)
            dst = regs(parts[1].split(',')[0]) if len(parts) > 1 else set()
            if dst & read:
                bad.append((i + 1, s))
            need -= 1
        n_checked += 1
    return n_checked, bad


if __name__ == '__main__':
    status = 0
    for p in sys.argv[1:]:
        n, bad = check(p)
        print(f'{p}: {n} statements opening with a DPP read checked, {len(bad)} violations')
        for line, what in bad:
            print(f'  line {line}: {what}')
        status |= bool(bad)
    sys.exit(status)
