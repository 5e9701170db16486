'use strict';
// The temporal denoiser following a skinned mesh through the drop-in: a NativeRenderer made with
// {frameColor: true} renders and denoises two frames with Denoise({temporal: true, followVertices: true}), binds
// a skin, poses it, renders the next frame and denoises it the same way.
//
// argv: JSON {sceneDir, dir: directory with joints.u32, weights.f32, bind.f32, palette.f32, mesh, width, height,
//             pipeline, iterations, out}
// stdout: JSON {uniform: [33 words of the last frame]}; the last call's PTX_BUF_DENOISE_HISTORY goes to
// `${out}.history.f32`, ReadDenoised() to `${out}.denoised.f32`.
const fs = require('fs');
const path = require('path');
const { NativeRenderer, addon, BUF } = require('../../pathtracerdemo_amd/js/NativeRenderer');
const { loadCompiledScene } = require('../../pathtracerdemo_amd/js/scene_io');

function load(file, Type) {
  const bytes = fs.readFileSync(file);
  return new Type(bytes.buffer.slice(bytes.byteOffset, bytes.byteOffset + bytes.byteLength));
}

async function main() {
  const req = JSON.parse(process.argv[2]);
  const world = loadCompiledScene(req.sceneDir);
  const f = (name, Type) => load(path.join(req.dir, name), Type);
  const r = new NativeRenderer(req.width, req.height, { pipeline: req.pipeline, device: 0, frameColor: true });
  await r.Initialize(world);
  const opts = { temporal: true, followVertices: true, iterations: req.iterations };
  for (let k = 0; k < 2; ++k) {
    r.Update();
    r.Render();
    r.Denoise(opts);
  }
  r.SetSkin(req.mesh, 0, f('joints.u32', Uint32Array), f('weights.f32', Float32Array), f('bind.f32', Float32Array));
  r.SkinVertices(req.mesh, f('palette.f32', Float32Array));
  r.Update();
  r.Render();
  r.Denoise(opts);
  const history = new Float32Array(req.width * req.height * 4);
  addon.readBuffer(r.Handle, BUF.DENOISE_HISTORY, history);
  fs.writeFileSync(`${req.out}.history.f32`, Buffer.from(history.buffer));
  fs.writeFileSync(`${req.out}.denoised.f32`, Buffer.from(r.ReadDenoised().buffer));
  const res = { uniform: Array.from(r.Uniform) };
  r.Destroy();
  process.stdout.write(JSON.stringify(res));
}
main().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
