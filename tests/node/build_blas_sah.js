'use strict';
// Building a BLAS on the GPU with the SAH builder through the drop-in: BuildBlas(..., {builder: 'sah'}) on a
// NativeRenderer without a world.
//
// argv: JSON {positions: file of f32, indices: file of u32, groups: [[first, count], ...], maxLeaf, out}
// stdout: JSON {nodes: [nodes per root], maxDepth, lbvhNodes: [nodes per root of {builder: 'lbvh'}],
//               defaultNodes: [... of no options], refused: [messages]}; the SAH roots, one after the other, go to
// `${out}.nodes.u32`, the reordered indices to `${out}.indices.u32`.
const fs = require('fs');
const { NativeRenderer } = require('../../pathtracerdemo_amd/js/NativeRenderer');

function load(file, Type) {
  const b = fs.readFileSync(file);
  return new Type(b.buffer.slice(b.byteOffset, b.byteOffset + b.byteLength));
}

function main() {
  const req = JSON.parse(process.argv[2]);
  const positions = load(req.positions, Float32Array);
  const indices = load(req.indices, Uint32Array);
  const r = new NativeRenderer(32, 32, { pipeline: 'reuse', device: 0 });
  const refused = [];
  for (const call of [() => r.BuildBlas(positions, indices, req.groups, req.maxLeaf, { builder: 'ploc' }),
    () => r.BuildBlas(positions, indices, req.groups, req.maxLeaf, { builder: 1 })]) {
    try { call(); refused.push(null); } catch (e) { refused.push(`${e.name}: ${e.message}`); }
  }
  const b = r.BuildBlas(positions, indices, req.groups, req.maxLeaf, { builder: 'sah' });
  const lbvh = r.BuildBlas(positions, indices, req.groups, req.maxLeaf, { builder: 'lbvh' });
  const dflt = r.BuildBlas(positions, indices, req.groups, req.maxLeaf);
  const total = b.roots.reduce((n, x) => n + x.length, 0);
  const nodes = new Uint32Array(total);
  let at = 0;
  for (const x of b.roots) { nodes.set(x, at); at += x.length; }
  fs.writeFileSync(`${req.out}.nodes.u32`, Buffer.from(nodes.buffer));
  fs.writeFileSync(`${req.out}.indices.u32`, Buffer.from(b.indices.buffer, b.indices.byteOffset, b.indices.byteLength));
  r.Destroy();
  process.stdout.write(JSON.stringify({
    nodes: b.roots.map((x) => x.length / 8), maxDepth: b.maxDepth, lbvhNodes: lbvh.roots.map((x) => x.length / 8),
    defaultNodes: dflt.roots.map((x) => x.length / 8), refused,
  }));
}
try { main(); } catch (e) { console.error(e.stack || String(e)); process.exit(1); }
